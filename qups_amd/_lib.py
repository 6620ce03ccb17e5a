"""ctypes binding of ``libqdas.so`` -- the only way the Python host reaches the HIP kernels.

Mirrors ``include/qdas.h`` one to one.  There is deliberately NO fallback: if the shared
library is missing or does not export a symbol, importing this module's :func:`lib`
raises; if no HIP device is present, plan creation fails with the HIP error text.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QDAS_LIB") or os.path.join(_HERE, "libqdas.so")   # QDAS_LIB: A/B builds for profiling

# ---- constants (include/qdas.h)
QDAS_F64, QDAS_F32, QDAS_F16 = 0, 1, 2
INTERP_FLAGS = {"nearest": 0, "linear": 1, "cubic": 2, "lanczos3": 3, "cubic_dev": 5}
FLAG_KEEP_RX, FLAG_KEEP_TX, FLAG_TPOSE = 8, 16, 32
MEM_HOST, MEM_DEVICE = 0, 1
KERNEL_AUTO, KERNEL_GENERIC, KERNEL_TILED = 0, 1, 2
KERNEL_NAMES = {KERNEL_GENERIC: "generic", KERNEL_TILED: "tiled"}
MAX_APOD = 6
QDAS_PRE_F32, QDAS_PRE_I16 = 0, 1
QDAS_CONV_FULL, QDAS_CONV_SAME, QDAS_CONV_VALID, QDAS_CONV_CAUSAL = 0, 1, 2, 3
QDAS_CONV_X_ONE_COLUMN, QDAS_CONV_X_ONE_SLICE, QDAS_CONV_Y_ONE_COLUMN, QDAS_CONV_Y_ONE_SLICE = 1, 2, 4, 8
PLAN_NO_RECIPROCAL, PLAN_JIT, PLAN_COPY_INPUTS, PLAN_NO_MIRROR, PLAN_MIRROR_SLAB, PLAN_NO_FOLD, PLAN_APPROX_SYMMETRY, PLAN_PREFOLDED = 1, 2, 4, 8, 16, 32, 64, 128
COH_SLSC_AVERAGE, COH_SLSC_ENSEMBLE, COH_DMAS, COH_COHFAC, COH_PCF = 1, 2, 3, 4, 5
QDAS_ENOCONV = 5
QDAS_ENOTLDS = 6
QDAS_EUNSUPPORTED = 2
RXAPOD_NONE, RXAPOD_ACCEPTANCE, RXAPOD_COSINE, RXAPOD_FNUMBER_PLANAR, RXAPOD_FNUMBER_ORIENTED = 0, 1, 2, 3, 4

# every symbol include/qdas.h declares (tests check the library exports all of them)
SYMBOLS = (
    "qdas_plan_create", "qdas_plan_execute", "qdas_plan_execute_frames", "qdas_plan_prepare_frames", "qdas_plan_delays",
    "qdas_plan_destroy", "qdas_plan_kernel", "qdas_plan_fallback_tiles", "qdas_plan_tile_shape", "qdas_plan_reciprocal", "qdas_plan_folded", "qdas_fold", "qdas_plan_symmetry_bound", "qdas_plan_mirror", "qdas_plan_kernel_name", "qdas_plan_set_timing",
    "qdas_plan_last_kernel_ms", "qdas_plan_create_sharded", "qdas_plan_execute_sharded", "qdas_plan_sharded_info", "qdas_plan_sharded_mirror",
    "qdas_plan_destroy_sharded", "qdas_DAS", "qdas_DASf", "qdas_DASh", "qdas_delays", "qdas_delaysf",
    "qdas_das_lut", "qdas_das_lut_last_kernel", "qdas_wsinterpd", "qdas_shift_sum", "qdas_greens", "qdas_convd", "qdas_convd_len", "qdas_permute3", "qdas_pre_plan_create", "qdas_pre_execute", "qdas_pre_plan_destroy", "qdas_pre_plan_one_pass", "qdas_last_error", "qdas_version", "qdas_device_malloc", "qdas_device_free", "qdas_device_trim", "qdas_device_copy", "qdas_iir", "qdas_device_info", "qdas_kernel_variant_build", "qdas_kernel_variant_prebuilt",
    "qdas_coherence", "qdas_eikonal", "qdas_eikonal_tables", "qdas_eikonal_last_passes", "qdas_eikonal_pass_cap", "qdas_adjoint", "qdas_migration",
    "qdas_pwznxcorr", "qdas_pwznxcorr_time_tile", "qdas_pwznxcorr_lds_bytes", "qdas_refocus", "qdas_refocus_work_bytes",
    "qdas_raypaths_slots", "qdas_raypaths_weights", "qdas_raypaths_integrate", "qdas_raypaths_backproject",
    "qdas_eikonal3", "qdas_eikonal3_tables", "qdas_eikonal3_work_bytes", "qdas_eikonal3_pass_cap",
    "qdas_scanconvert", "qdas_demod", "qdas_demod_len", "qdas_resample", "qdas_resample_len", "qdas_upfirdn_len",
    "qdas_fdtd", "qdas_fdtd_tiles", "qdas_fdtd_tile_lists", "qdas_fdtd_lossy", "qdas_fdtd_nonlinear",
    "qdas_fdtd3", "qdas_fdtd3_bricks", "qdas_fdtd3_brick_lists",
)


class Sizes(C.Structure):
    _fields_ = [("T", C.c_uint64), ("N", C.c_uint64), ("M", C.c_uint64),
                ("I1", C.c_uint64), ("I2", C.c_uint64), ("I3", C.c_uint64), ("S", C.c_uint64),
                ("flag", C.c_int32), ("VS", C.c_int32), ("DV", C.c_int32), ("dtype", C.c_int32)]


class Desc(C.Structure):
    _fields_ = [("sz", Sizes), ("fs", C.c_double), ("fmod", C.c_double),
                ("Pi", C.c_void_p), ("Pr", C.c_void_p), ("Pv", C.c_void_p), ("Nv", C.c_void_p),
                ("apod", C.c_void_p), ("cinv", C.c_void_p), ("acstride", C.POINTER(C.c_uint64)),
                ("mem", C.c_int32), ("apod_real", C.c_int32), ("kernel", C.c_int32), ("device", C.c_int32),
                ("i_begin", C.c_uint64), ("i_count", C.c_uint64), ("y_ld", C.c_uint64),
                ("rx_apod_kind", C.c_int32), ("plan_flags", C.c_int32), ("rx_apod_p", C.c_double * 2),
                ("rx_normals", C.c_void_p)]


class LutDesc(C.Structure):
    _fields_ = [("T", C.c_uint64), ("N", C.c_uint64), ("M", C.c_uint64), ("I", C.c_uint64),
                ("flag", C.c_int32), ("dtype", C.c_int32), ("omega", C.c_double),
                ("tau_rx", C.c_void_p), ("tau_tx", C.c_void_p), ("w", C.c_void_p),
                ("wstride", C.c_uint64 * 3), ("w_real", C.c_int32), ("reserved", C.c_int32), ("I1", C.c_uint64)]


class WsDesc(C.Structure):
    _fields_ = [("T", C.c_uint64), ("x_tstride", C.c_uint64), ("ndim", C.c_int32), ("flag", C.c_int32), ("dtype", C.c_int32),
                ("w_real", C.c_int32), ("size", C.c_uint64 * 8), ("tstride", C.c_int64 * 8), ("xstride", C.c_int64 * 8),
                ("wstride", C.c_int64 * 8), ("sum", C.c_uint8 * 8), ("omega", C.c_double), ("extrap", C.c_double),
                ("t", C.c_void_p), ("w", C.c_void_p), ("x", C.c_void_p), ("ystride", C.c_int64 * 8), ("lane_dim", C.c_int32), ("reserved", C.c_int32)]


class FoldDesc(C.Structure):
    _fields_ = [("T", C.c_uint64), ("N", C.c_uint64), ("strN", C.c_uint64), ("strM", C.c_uint64), ("dtype", C.c_int32), ("device", C.c_int32), ("wtab", C.c_void_p)]


class IirDesc(C.Structure):
    _fields_ = [("T", C.c_uint64), ("K", C.c_uint64), ("nsec", C.c_int32), ("dtype", C.c_int32), ("cplx", C.c_int32), ("device", C.c_int32),
                ("gain", C.c_double), ("sos", C.POINTER(C.c_double))]


class GreensDesc(C.Structure):
    _fields_ = [("S", C.c_uint64), ("T", C.c_uint64), ("N", C.c_uint64), ("M", C.c_uint64), ("I", C.c_uint64),
                ("En", C.c_int32), ("Em", C.c_int32), ("interp", C.c_int32), ("dtype", C.c_int32),
                ("s0", C.c_double), ("t0", C.c_double), ("fs", C.c_double), ("fsr", C.c_double), ("cinv", C.c_double),
                ("R0", C.c_double), ("Ps", C.c_void_p), ("a", C.c_void_p), ("Pr", C.c_void_p), ("Pv", C.c_void_p),
                ("x", C.c_void_p), ("device", C.c_int32), ("reserved", C.c_int32)]


class PreDesc(C.Structure):
    _fields_ = [("T", C.c_uint64), ("K", C.c_uint64), ("Nfft", C.c_uint64), ("in_type", C.c_int32), ("device", C.c_int32),
                ("fs", C.c_double), ("t0", C.c_double), ("fdown", C.c_double)]


class ShiftDesc(C.Structure):
    _fields_ = [("T", C.c_uint64), ("To", C.c_uint64), ("N", C.c_uint64), ("M", C.c_uint64), ("Mo", C.c_uint64), ("F", C.c_uint64),
                ("flag", C.c_int32), ("dtype", C.c_int32), ("cplx", C.c_int32), ("w_real", C.c_int32), ("device", C.c_int32), ("tpad", C.c_int32),
                ("shift", C.c_void_p), ("w", C.c_void_p)]


class ConvdDesc(C.Structure):
    _fields_ = [("C", C.c_uint64), ("M", C.c_uint64), ("N", C.c_uint64), ("S", C.c_uint64), ("dtype", C.c_int32), ("cplx", C.c_int32),
                ("shape", C.c_int32), ("bcast", C.c_int32), ("device", C.c_int32), ("y_real", C.c_int32)]


class CoherenceDesc(C.Structure):
    _fields_ = [("method", C.c_int32), ("dtype", C.c_int32), ("cplx", C.c_int32), ("device", C.c_int32),
                ("N", C.c_uint64), ("K", C.c_uint64), ("strideN", C.c_int64), ("strideK", C.c_int64),
                ("size", C.c_uint64 * 3), ("stride", C.c_int64 * 3), ("lag_lo", C.c_uint64), ("lag_hi", C.c_uint64),
                ("lags", C.POINTER(C.c_int64)), ("nlags", C.c_uint64), ("gamma", C.c_double)]


class EikonalDesc(C.Structure):
    _fields_ = [("C1", C.c_uint64), ("C2", C.c_uint64), ("K", C.c_uint64), ("npts", C.c_uint64), ("set_begin", C.POINTER(C.c_uint64)),
                ("dp", C.c_double), ("base", C.c_int32), ("device", C.c_int32), ("max_passes", C.c_uint32), ("reserved", C.c_uint32),
                ("I", C.c_uint64)]


class Eikonal3Desc(C.Structure):
    _fields_ = [("C1", C.c_uint64), ("C2", C.c_uint64), ("C3", C.c_uint64), ("K", C.c_uint64), ("npts", C.c_uint64),
                ("set_begin", C.POINTER(C.c_uint64)), ("dp", C.c_double), ("base", C.c_int32), ("device", C.c_int32),
                ("max_passes", C.c_uint32), ("reserved", C.c_uint32), ("I", C.c_uint64), ("queue", C.c_void_p)]


class AdjointDesc(C.Structure):
    _fields_ = [("I", C.c_uint64), ("N", C.c_uint64), ("M", C.c_uint64), ("V", C.c_uint64), ("Ksel", C.c_uint64),
                ("Pi", C.c_void_p), ("Pr", C.c_void_p), ("Pt", C.c_void_p), ("cinv", C.c_void_p), ("cinv_count", C.c_uint64),
                ("freq", C.c_void_p), ("del_tx", C.c_void_p), ("apod_tx", C.c_void_p), ("a_n", C.c_void_p), ("a_m", C.c_void_p),
                ("keep_rx", C.c_int32), ("keep_tx", C.c_int32), ("dtype", C.c_int32), ("device", C.c_int32)]


class MigrationDesc(C.Structure):
    _fields_ = [("T", C.c_uint64), ("N", C.c_uint64), ("M", C.c_uint64), ("frames", C.c_uint64), ("F", C.c_uint64), ("K", C.c_uint64),
                ("fs", C.c_double), ("fmod", C.c_double), ("t0", C.c_double), ("c0", C.c_double), ("pitch", C.c_double),
                ("flag", C.c_int32), ("keep_tx", C.c_int32), ("jacobian", C.c_int32), ("device", C.c_int32),
                ("tau", C.c_void_p), ("gamma", C.c_void_p)]


class PwznxcorrDesc(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("cplx", C.c_int32), ("device", C.c_int32), ("zero", C.c_int32), ("norm", C.c_int32), ("pad", C.c_int32),
                ("T", C.c_uint64), ("N", C.c_uint64), ("W", C.c_uint64), ("nlags", C.c_uint64), ("bsize", C.c_uint64 * 2),
                ("xl_strideN", C.c_int64), ("xl_bstride", C.c_int64 * 2), ("xr_strideN", C.c_int64), ("xr_bstride", C.c_int64 * 2),
                ("y_strideN", C.c_int64), ("y_bstride", C.c_int64 * 2), ("y_strideL", C.c_int64)]


class RefocusDesc(C.Structure):
    _fields_ = [("T", C.c_uint64), ("N", C.c_uint64), ("V", C.c_uint64), ("M", C.c_uint64), ("frames", C.c_uint64),
                ("fs", C.c_double), ("t0_out", C.c_double), ("device", C.c_int32), ("one_t0", C.c_int32),
                ("t0", C.c_void_p), ("queue", C.c_void_p)]


class RaypathsDesc(C.Structure):
    _fields_ = [("X", C.c_uint64), ("Z", C.c_uint64), ("J", C.c_uint64), ("F", C.c_uint64),
                ("xstride", C.c_int64), ("zstride", C.c_int64), ("pa_stride", C.c_int64), ("pb_stride", C.c_int64),
                ("dtype", C.c_int32), ("device", C.c_int32),
                ("xg", C.c_void_p), ("zg", C.c_void_p), ("pa", C.c_void_p), ("pb", C.c_void_p), ("queue", C.c_void_p)]


SC_PRE_NONE, SC_PRE_ABS, SC_PRE_DB = 0, 1, 2


class ScanconvertDesc(C.Structure):
    _fields_ = [("R", C.c_uint64), ("A", C.c_uint64), ("E", C.c_uint64), ("Z", C.c_uint64), ("X", C.c_uint64), ("Y", C.c_uint64), ("P", C.c_uint64),
                ("sr", C.c_int64), ("sa", C.c_int64), ("se", C.c_int64), ("sp", C.c_int64),
                ("dtype", C.c_int32), ("cplx", C.c_int32), ("pre", C.c_int32), ("device", C.c_int32),
                ("origin", C.c_double * 3), ("fill", C.c_double), ("db_floor", C.c_double),
                ("r", C.c_void_p), ("a", C.c_void_p), ("e", C.c_void_p), ("x", C.c_void_p), ("y", C.c_void_p), ("z", C.c_void_p),
                ("queue", C.c_void_p)]


DEMOD_I16, DEMOD_F32, DEMOD_C64, DEMOD_F64, DEMOD_C128 = 0, 1, 2, 3, 4
DEMOD_MAX_K, DEMOD_MAX_R, DEMOD_TILE = 1024, 4096, 256


class DemodDesc(C.Structure):
    _fields_ = [("T", C.c_uint64), ("C", C.c_uint64), ("K", C.c_uint64), ("R", C.c_uint64), ("x_ld", C.c_uint64), ("out_ld", C.c_uint64),
                ("in_type", C.c_int32), ("out_half", C.c_int32), ("device", C.c_int32), ("reserved", C.c_int32),
                ("fc_over_fs", C.c_double), ("step", C.c_double), ("cyc0", C.c_void_p), ("gdiv", C.c_uint64), ("G", C.c_uint64),
                ("queue", C.c_void_p)]


RESAMPLE_I16, RESAMPLE_F32, RESAMPLE_C64, RESAMPLE_F64, RESAMPLE_C128 = 0, 1, 2, 3, 4
RESAMPLE_ZERO, RESAMPLE_ODD = 0, 1
RESAMPLE_MAX_K, RESAMPLE_MAX_PQ = 8192, 4096


class ResampleDesc(C.Structure):
    _fields_ = [("T", C.c_uint64), ("C", C.c_uint64), ("K", C.c_uint64), ("J", C.c_uint64), ("p", C.c_uint64), ("q", C.c_uint64), ("off", C.c_uint64),
                ("x_ld", C.c_uint64), ("out_ld", C.c_uint64), ("in_type", C.c_int32), ("edge", C.c_int32), ("device", C.c_int32), ("reserved", C.c_int32),
                ("queue", C.c_void_p)]


FDTD_TZ, FDTD_TX, FDTD_ZERO = 64, 16, 1


class FdtdDesc(C.Structure):
    _fields_ = [("Nz", C.c_uint64), ("Nx", C.c_uint64), ("V", C.c_uint64), ("Nt", C.c_uint64), ("ld", C.c_uint64), ("vstride", C.c_uint64),
                ("M", C.c_uint64), ("Ts", C.c_uint64), ("N", C.c_uint64), ("rec_st", C.c_uint64), ("rec_sn", C.c_uint64), ("rec_sv", C.c_uint64),
                ("dt_h", C.c_double), ("inv_h", C.c_double), ("dtype", C.c_int32), ("order", C.c_int32), ("device", C.c_int32), ("flags", C.c_int32),
                ("queue", C.c_void_p)]


FDTD_ARGS = ("p", "uz", "ux", "rz", "rx", "c2", "rho", "dtrz", "dtrx", "az", "azs", "ax", "axs", "s", "src_wz", "src_wx",
             "src_node", "src_start", "src_list", "sen_node", "sen_start", "sen_list", "rec")


class FdtdArgs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in FDTD_ARGS]


FDTD_LOSS_STOKES, FDTD_LOSS_RELAX, FDTD_MAX_L = 1, 2, 4


class FdtdLoss(C.Structure):
    _fields_ = [("mode", C.c_int32), ("L", C.c_int32), ("g", C.c_double * 4), ("E", C.c_double * 4), ("kap", C.c_void_p), ("e", C.c_void_p)]


FDTD_NL_NO_CONVECTIVE = 1


class FdtdNl(C.Structure):
    _fields_ = [("bq", C.c_void_p), ("flags", C.c_int32)]


FDTD3_TZ, FDTD3_TX, FDTD3_TY, FDTD3_ZERO = 64, 8, 8, 1


class Fdtd3Desc(C.Structure):
    _fields_ = [("Nz", C.c_uint64), ("Nx", C.c_uint64), ("Ny", C.c_uint64), ("V", C.c_uint64), ("Nt", C.c_uint64), ("ld", C.c_uint64), ("pstride", C.c_uint64),
                ("vstride", C.c_uint64), ("M", C.c_uint64), ("Ts", C.c_uint64), ("N", C.c_uint64), ("rec_st", C.c_uint64), ("rec_sn", C.c_uint64),
                ("rec_sv", C.c_uint64), ("dt_h", C.c_double), ("inv_h", C.c_double), ("dtype", C.c_int32), ("order", C.c_int32), ("device", C.c_int32),
                ("flags", C.c_int32), ("queue", C.c_void_p)]


FDTD3_ARGS = ("p", "uz", "ux", "uy", "rz", "rx", "ry", "c2", "rho", "dtrz", "dtrx", "dtry", "az", "azs", "ax", "axs", "ay", "ays", "s", "src_wz", "src_wx",
              "src_wy", "src_node", "src_start", "src_list", "sen_node", "sen_start", "sen_list", "rec")


class Fdtd3Args(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in FDTD3_ARGS]


class QdasError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libqdas error {code}: {msg}")
        self.code = code
        self.message = msg


_LIB = None


def lib():
    """Load ``libqdas.so`` (built in-tree by ``__graft_entry__.build()`` / ``make -C qups_amd/csrc``)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` (or `make -C qups_amd/csrc`). There is no CPU fallback in this package.")
    try:  # share torch's HIP runtime (same SONAME libamdhip64.so.7) when torch is in the process
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - the library also works without torch (MEX / C callers)
        pass
    L = C.CDLL(LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(L, s)]
    if missing:
        raise ImportError(f"{LIB_PATH} does not export {missing}")
    L.qdas_last_error.restype = C.c_char_p
    L.qdas_plan_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(Desc)]
    L.qdas_plan_execute.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.qdas_plan_execute_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    L.qdas_plan_prepare_frames.argtypes = [C.c_void_p, C.c_uint64]
    L.qdas_plan_delays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.qdas_plan_destroy.argtypes = [C.c_void_p]
    L.qdas_plan_destroy.restype = None
    L.qdas_plan_kernel.argtypes = [C.c_void_p]
    L.qdas_plan_fallback_tiles.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.qdas_plan_tile_shape.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.qdas_plan_reciprocal.argtypes = [C.c_void_p]
    L.qdas_plan_mirror.argtypes = [C.c_void_p]
    L.qdas_plan_folded.argtypes = [C.c_void_p]
    L.qdas_fold.argtypes = [C.POINTER(FoldDesc), C.c_void_p, C.c_void_p, C.c_void_p]
    L.qdas_plan_symmetry_bound.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.qdas_plan_kernel_name.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.qdas_plan_set_timing.argtypes = [C.c_void_p, C.c_int]
    L.qdas_plan_last_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.qdas_plan_create_sharded.argtypes = [C.POINTER(C.c_void_p), C.POINTER(Desc), C.c_int, C.POINTER(C.c_int)]
    L.qdas_plan_execute_sharded.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.qdas_plan_sharded_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
    L.qdas_plan_sharded_mirror.argtypes = [C.c_void_p]
    L.qdas_plan_destroy_sharded.argtypes = [C.c_void_p]
    L.qdas_plan_destroy_sharded.restype = None
    L.qdas_das_lut.argtypes = [C.POINTER(LutDesc), C.c_void_p, C.c_void_p, C.c_void_p]
    L.qdas_wsinterpd.argtypes = [C.POINTER(WsDesc), C.c_void_p, C.c_void_p]
    L.qdas_greens.argtypes = [C.POINTER(GreensDesc), C.c_void_p, C.c_void_p]
    L.qdas_convd.argtypes = [C.POINTER(ConvdDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.qdas_permute3.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p]
    L.qdas_coherence.argtypes = [C.POINTER(CoherenceDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.qdas_eikonal.argtypes = [C.POINTER(EikonalDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.qdas_eikonal_tables.argtypes = [C.POINTER(EikonalDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.qdas_eikonal_last_passes.argtypes = []
    L.qdas_eikonal_pass_cap.argtypes = [C.c_uint64, C.c_uint64]
    L.qdas_eikonal_pass_cap.restype = C.c_uint32
    L.qdas_eikonal3_pass_cap.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
    L.qdas_eikonal3_pass_cap.restype = C.c_uint32
    L.qdas_eikonal3_work_bytes.argtypes = [C.POINTER(Eikonal3Desc), C.POINTER(C.c_uint64)]
    L.qdas_eikonal3.argtypes = [C.POINTER(Eikonal3Desc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32)]
    L.qdas_eikonal3_tables.argtypes = [C.POINTER(Eikonal3Desc), C.c_void_p, C.c_void_p, C.c_void_p]
    L.qdas_adjoint.argtypes = [C.POINTER(AdjointDesc), C.c_void_p, C.c_void_p, C.c_void_p]
    L.qdas_migration.argtypes = [C.POINTER(MigrationDesc), C.c_void_p, C.c_void_p, C.c_void_p]
    L.qdas_pwznxcorr.argtypes = [C.POINTER(PwznxcorrDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p]
    L.qdas_pwznxcorr_time_tile.argtypes = []
    L.qdas_pwznxcorr_lds_bytes.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_uint64]
    L.qdas_pwznxcorr_lds_bytes.restype = C.c_uint64
    L.qdas_refocus_work_bytes.argtypes = [C.POINTER(RefocusDesc), C.POINTER(C.c_uint64)]
    L.qdas_refocus.argtypes = [C.POINTER(RefocusDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    L.qdas_raypaths_slots.argtypes = [C.c_uint64, C.c_uint64]
    L.qdas_raypaths_slots.restype = C.c_uint64
    L.qdas_raypaths_weights.argtypes = [C.POINTER(RaypathsDesc), C.c_void_p, C.c_void_p, C.c_void_p]
    L.qdas_raypaths_integrate.argtypes = [C.POINTER(RaypathsDesc), C.c_void_p, C.c_void_p, C.c_void_p]
    L.qdas_raypaths_backproject.argtypes = [C.POINTER(RaypathsDesc), C.c_void_p, C.c_void_p, C.c_void_p]
    L.qdas_scanconvert.argtypes = [C.POINTER(ScanconvertDesc), C.c_void_p, C.c_void_p]
    L.qdas_demod.argtypes = [C.POINTER(DemodDesc), C.c_void_p, C.c_void_p, C.c_void_p]
    L.qdas_demod_len.argtypes = [C.c_uint64, C.c_uint64]
    L.qdas_demod_len.restype = C.c_uint64
    L.qdas_resample.argtypes = [C.POINTER(ResampleDesc), C.c_void_p, C.c_void_p, C.c_void_p]
    L.qdas_resample_len.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
    L.qdas_resample_len.restype = C.c_uint64
    L.qdas_upfirdn_len.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64]
    L.qdas_upfirdn_len.restype = C.c_uint64
    L.qdas_fdtd.argtypes = [C.POINTER(FdtdDesc), C.POINTER(FdtdArgs)]
    L.qdas_fdtd_lossy.argtypes = [C.POINTER(FdtdDesc), C.POINTER(FdtdArgs), C.POINTER(FdtdLoss)]
    L.qdas_fdtd_nonlinear.argtypes = [C.POINTER(FdtdDesc), C.POINTER(FdtdArgs), C.POINTER(FdtdLoss), C.POINTER(FdtdNl)]
    L.qdas_fdtd_tiles.argtypes = [C.c_uint64, C.c_uint64]
    L.qdas_fdtd_tiles.restype = C.c_uint64
    L.qdas_fdtd_tile_lists.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.qdas_fdtd3.argtypes = [C.POINTER(Fdtd3Desc), C.POINTER(Fdtd3Args)]
    L.qdas_fdtd3_bricks.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
    L.qdas_fdtd3_bricks.restype = C.c_uint64
    L.qdas_fdtd3_brick_lists.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.qdas_convd_len.argtypes = [C.c_uint64, C.c_uint64, C.c_int]
    L.qdas_convd_len.restype = C.c_uint64
    L.qdas_shift_sum.argtypes = [C.POINTER(ShiftDesc), C.c_void_p, C.c_void_p, C.c_void_p]
    L.qdas_pre_plan_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(PreDesc)]
    L.qdas_pre_execute.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.qdas_pre_plan_destroy.argtypes = [C.c_void_p]
    L.qdas_pre_plan_destroy.restype = None
    L.qdas_pre_plan_one_pass.argtypes = [C.c_void_p]
    L.qdas_kernel_variant_build.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    L.qdas_kernel_variant_prebuilt.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    L.qdas_device_malloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_int]
    L.qdas_device_free.argtypes = [C.c_void_p, C.c_int]
    L.qdas_device_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int]
    L.qdas_device_trim.argtypes = []
    L.qdas_device_info.argtypes = [C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                   C.POINTER(C.c_uint64)]
    vp, u64p = C.c_void_p, C.POINTER(C.c_uint64)
    for name in ("qdas_DAS", "qdas_DASf", "qdas_DASh"):
        getattr(L, name).argtypes = [C.POINTER(Sizes), vp, vp, vp, vp, vp, vp, vp, u64p, vp, vp, vp]
    L.qdas_delays.argtypes = [C.POINTER(Sizes), vp, vp, vp, vp, vp, C.c_double, vp]
    L.qdas_delaysf.argtypes = [C.POINTER(Sizes), vp, vp, vp, vp, vp, C.c_float, vp]
    _LIB = L
    return L


def check(rc: int):
    if rc:
        raise QdasError(rc, (lib().qdas_last_error() or b"").decode(errors="replace"))


def device_info(device: int = -1) -> dict:
    name = C.create_string_buffer(256)
    cu, clk, mem = C.c_int(), C.c_int(), C.c_uint64()
    check(lib().qdas_device_info(device, name, 256, C.byref(cu), C.byref(clk), C.byref(mem)))
    return {"name": name.value.decode(), "cu_count": cu.value, "clock_khz": clk.value, "hbm_bytes": mem.value}
