"""qups_amd -- MI355X-native delay-and-sum beamforming engine.

A from-scratch drop-in for ONE hot path of thorstone25/qups: ``UltrasoundSystem.DAS`` /
``bfDAS`` -> ``das_spec`` -> the ``DAS*`` device kernels.
The compute lives in ``libqdas.so`` (hand-written HIP for gfx950, C ABI in ``include/qdas.h``);
this package is the host-side mirror of the reference's interface for that path.
"""
from .das_spec import (DasError, DasPlan, DasProblem, MultiDevicePlan, build_problem, clear_plan_cache, das_spec, parse_options,
                       plan_cache_info, problem_key)  # noqa: F401

from .interpd import das_lut, sample2sep, wsinterpd2  # noqa: F401,E402
from . import apodization  # noqa: F401,E402
from . import preproc  # noqa: F401,E402
from .convd import convd, sosfilt  # noqa: F401,E402
from .coherence import cohfac, dmas, pcf, slsc  # noqa: F401,E402
from .correlator import pwznxcorr  # noqa: F401,E402
from .eikonal import msfm, msfm3d  # noqa: F401,E402
from . import adjoint  # noqa: F401,E402  (the module: adjoint.adjoint is the call, a function of the same name would shadow it)
from . import migration  # noqa: F401,E402
from . import refocus  # noqa: F401,E402  (the module: refocus.refocus is the call)
from .raypaths import globalAverageC, rayPaths, ray_backproject, ray_integrals, ray_sart, wbilerpg  # noqa: F401,E402
from .scanconvert import scan_convert, scan_convert3  # noqa: F401,E402
from .demod import demod  # noqa: F401,E402  (the call, under the module's name: the module itself is importlib.import_module("qups_amd.demod"))
from .resample import filtfilt, resample, resample_taps, upfirdn  # noqa: F401,E402  (resample is the call; the module is importlib.import_module("qups_amd.resample"))
from . import fdtd  # noqa: F401,E402  (the module: fdtd.fdtd is the call, UltrasoundSystem.fdtdSim the wrapper)
from . import fdtd3  # noqa: F401,E402  (fdtd3.fdtd3: the same through volumes)
from .ultrasound import ChannelData, Scan, Sequence, Transducer, UltrasoundSystem  # noqa: F401,E402

__all__ = ["das_spec", "DasPlan", "MultiDevicePlan", "DasProblem", "DasError", "build_problem", "parse_options", "das_lut", "sample2sep",
           "wsinterpd2", "convd", "slsc", "dmas", "cohfac", "pcf", "pwznxcorr", "msfm", "msfm3d", "adjoint", "migration", "refocus", "wbilerpg", "ray_integrals", "ray_backproject", "ray_sart", "rayPaths", "globalAverageC", "scan_convert", "scan_convert3", "demod", "resample", "resample_taps", "upfirdn", "filtfilt", "fdtd", "fdtd3", "UltrasoundSystem", "Transducer", "Sequence", "Scan", "ChannelData"]
