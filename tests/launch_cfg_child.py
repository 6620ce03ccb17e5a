"""Child process of tests/test_gpu_launch_cfg.py: one tiny plan per reachable family of the fused kernel's launch configurations, executed with
``QDAS_KERNEL_CENSUS`` set (the census file name is read once per process, hence a process of its own).  Prints one JSON object:
``{family: {"census": [[configuration, probe], ...], "err": max|tiled - generic| / max|generic|}}``.

The census lists an instantiation (configuration, interpolator, sample bytes, remodulation, table, probe) once per PROCESS, so families that share a
launch configuration use different interpolators: every family's own launch is a new line.  A probe that an earlier family already ran with the same
interpolator and data type does not show again (the probes of the two general-mode streams)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from qups_amd import DasPlan, build_problem, das_lut, parse_options      # noqa: E402
from qups_amd.das_spec import _cast_data, _colmajor                      # noqa: E402
from tests.cases import cinv_f32, make_case, rel_err                     # noqa: E402

CENSUS = os.environ["QDAS_KERNEL_CENSUS"]
N, T, I1, I2 = 16, 512, 64, 32


def census_lines():
    if not os.path.exists(CENSUS):
        return []
    with open(CENSUS) as fh:
        return [ln.split() for ln in fh if ln.strip()]


def new_pairs(seen):
    """(configuration, probe) of the census lines written since ``seen`` lines"""
    lines = census_lines()
    return sorted({(int(p[0]), int(p[5])) for p in lines[seen:]}), len(lines)


def to_np(y, prec):
    y = y.to(torch.complex128 if prec == "double" else torch.complex64)
    return y.cpu().numpy().reshape(-1)


def run_plan(seq, interp, prec="single", F=1, fun="DAS", **kw):
    """the plan on the fused kernel (kernel=2) against the same plan forced to the generic kernel (kernel=1)"""
    case = make_case(seq=seq, interp=interp, seed=7, N=N, M=N, I1=I1, I2=I2, T=T, data="noise")
    rng = np.random.default_rng(8)
    xs = np.stack([case["x"]] + [(rng.standard_normal(case["x"].shape) + 1j * rng.standard_normal(case["x"].shape)).astype(np.complex64)
                                 for _ in range(F - 1)], axis=3) if F > 1 else case["x"]
    xt = torch.from_numpy(np.ascontiguousarray(xs))
    opts = parse_options(xt, list(case["opt"]) + ["interp", interp, "input-precision", prec])
    prob = build_problem(fun, case["Pi"], case["Pr"], case["Pv"], case["Nv"], tuple(xt.shape), case["t0"], case["fs"], case["c"], opts)
    xc = _colmajor(_cast_data(xt, prob.prec, torch.device("cuda:0")))
    out = []
    for kernel in (2, 1):
        with DasPlan(prob, kernel=kernel, **kw) as plan:
            y = to_np(plan.execute_colmajor(xc, F), prec)
            torch.cuda.synchronize()
            assert plan.kernel == ("tiled" if kernel == 2 else "generic"), plan.kernel_name()
            if kernel == 2:
                assert plan.fallback_tiles() == 0, plan.kernel_name()      # (a tile redone by the generic kernel would compare that kernel with itself)
        out.append(y)
    return rel_err(out[0], out[1])


def run_lut(interp):
    """table-driven delays (qdas_das_lut) of a full-synthetic-aperture acquisition: the fused kernel against the one-thread-per-pixel kernel"""
    from oracle import das_oracle as O
    case = make_case(seq="FSA", interp=interp, seed=7, N=N, I1=I1, I2=I2, T=T, data="noise")
    dv, dr = O.tx_rx_distances(case["Pi"], case["Pr"], case["Pv"], case["Nv"], case["VS"], case["DV"])
    c = cinv_f32(case["c"])
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    tau_tx = f32((dv[:, :, :, 0, :] / c - case["t0"]) * case["fs"])[:, :, 0]
    tau_rx = f32(dr[:, :, :, :, 0] / c * case["fs"])[:, :, 0]
    out = []
    for generic in (False, True):
        if generic:
            os.environ["QDAS_LUT_GENERIC"] = "1"
        y = das_lut(torch.from_numpy(case["x"]), tau_rx, tau_tx, interp=interp, prec="single")
        torch.cuda.synchronize()
        os.environ.pop("QDAS_LUT_GENERIC", None)
        assert das_lut.last_kernel == ("generic" if generic else "tiled"), das_lut.last_kernel
        out.append(y.cpu().numpy().reshape(-1))
    return rel_err(out[0], out[1])


FAMILIES = [
    ("fp32 general",              lambda: run_plan("PW", "cubic", mirror=False)),
    ("fp16 general",              lambda: run_plan("PW", "cubic", prec="halfT", mirror=False)),
    ("fp64",                      lambda: run_plan("PW", "cubic", prec="double")),
    ("BF",                        lambda: run_plan("PW", "linear", fun="BF")),
    ("table-driven fp32",         lambda: run_lut("cubic")),
    ("folded",                    lambda: run_plan("FSA", "cubic", mirror=False)),
    ("folded, lateral mirror",    lambda: run_plan("FSA", "lanczos3")),
    ("general, lateral mirror",   lambda: run_plan("PW", "lanczos3")),
    ("fp16 reciprocal, no fold",  lambda: run_plan("FSA", "cubic", prec="halfT", mirror=False, fold=False)),
    ("2-frame stream",            lambda: run_plan("PW", "cubic", F=2, mirror=False)),
    ("4-frame stream",            lambda: run_plan("PW", "linear", F=4, mirror=False)),
    ("2-frame folded stream",     lambda: run_plan("FSA", "lanczos3", F=2, mirror=False)),
]


def main():
    torch.cuda.set_device(0)
    res, seen = {}, 0
    for name, fn in FAMILIES:
        err = fn()
        pairs, seen = new_pairs(seen)
        res[name] = {"census": [list(p) for p in pairs], "err": err}
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
