"""Memory-safety properties of every device entry that a parity test cannot see (helpers: tests/guards.py).

1. Guarded outputs.  Each case runs once unguarded (so torch's allocator holds a correct stale image of the same size), then with every
   ``torch.empty`` / ``empty_like`` / ``empty_strided`` of the wrapper replaced by a 0xFF-filled buffer between two 64 KiB bands of 0xFF: the bands must
   survive (nothing stored outside the output), no scalar of the returned output may still be 0xFF (everything written by THIS call), and the result
   must pass the parity its home test file asserts -- same oracle, same bound, imported from there.
2. Poisoned halos.  Every input that can be handed over as a device tensor sits in a larger buffer whose surroundings are 0, NaN and Inf in turn: the three
   results must be bit-identical.  Out of reach: positions, delay tables, weights and filters that a wrapper or a plan takes as HOST arrays and copies into
   allocations of its own (the geometry and apodization of a DasPlan, and with them ``plan.delays()``, which reads nothing else; ``tau`` / ``gamma`` of
   migration; the geometry of bfAdjoint; every argument of ``greens_kernel``, which uploads host arrays itself): for DAS plans, migration and adjoint the
   haloed input is the channel data, and greens and delays have no halo case.
   This sees out-of-bounds reads whose values reach arithmetic (0 x Inf = NaN).  It CANNOT see reads whose value is discarded by a select: those are
   legal by the kernels' contract (csrc/tile_staging.h) and invisible from the host.
3. Isolation.  Where outputs separate by construction (kept dimensions, one image per transmit, one value per pixel), a NaN / Inf trace must change
   nothing but its own slice, bit for bit: "select, not multiply".

The library's own arenas (csrc/scratch.hip) and plan scratch are not torch tensors: tests/test_gpu_scratch.py poisons them instead.  Not covered: stores
further than 64 KiB from the output."""
import collections
import functools
import os

import numpy as np
import pytest
import torch

from tests import guards as GD
from tests.cases import cinv_f32, make_case, rel_err

pytestmark = pytest.mark.gpu

SUMMARY = collections.OrderedDict()          # entry -> [cases, bytes guarded]
ENTRY_OF = {}                                # test function -> entry


def entry(name):
    def deco(f):
        ENTRY_OF[f.__name__] = name
        return f
    return deco


def _count(name, g):
    s = SUMMARY.setdefault(name, [0, 0])
    s[0] += 1
    s[1] += g.nbytes


def guarded(name, fn, monkeypatch, outputs=None, require=True, all_written=False):
    """``fn()`` once unguarded (dropped: the allocator's free list now holds a correct stale result), then guarded and checked.  ``outputs(r)``: the tensors
    of the result that must alias a guarded buffer (default: the result itself); ``require=False``: the wrapper post-processes its output in torch, only the bands
    are checked."""
    r0 = fn()
    torch.cuda.synchronize()
    del r0
    with GD.guard_outputs(monkeypatch) as g:
        r = fn()
        outs = r if outputs is None else outputs(r)
        n = g.check(*(outs if isinstance(outs, (tuple, list)) else [outs]), all_written=all_written)
    assert len(g.bufs) >= 1, f"{name}: the wrapper allocated nothing through torch.empty"
    if require:
        assert n >= 1, f"{name}: the result aliases no guarded buffer"
    _count(name, g)
    return r


def bits(t):
    """the tensor's bit pattern as integers (NaN compares equal to itself)"""
    t = t.contiguous()
    if t.is_complex():
        t = t.reshape(-1).view(GD._REAL[t.dtype])
    return t.view(GD._INT[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def _np(t):
    return (t.to(torch.complex128) if t.is_complex() else t).cpu().numpy()


FILLS = (0, "nan", "inf")


def halo_runs(fn, tensors):
    """fn(*tensors) with every tensor haloed by 0 / NaN / Inf: the three results, asserted bit-identical"""
    outs = []
    for fill in FILLS:
        hs = [None if t is None else (GD.haloed(t, fill) if t.is_contiguous() else GD.haloed_view(t, fill)) for t in tensors]
        r = fn(*hs)
        torch.cuda.synchronize()
        outs.append(r)
    tup = lambda r: tuple(r) if isinstance(r, (tuple, list)) else (r,)
    for fill, r in zip(FILLS[1:], outs[1:]):
        assert len(tup(r)) == len(tup(outs[0])) and all(same_bits(a, b) for a, b in zip(tup(outs[0]), tup(r))), \
            f"the result depends on what surrounds its inputs (fill {fill})"
    return outs[0]


# ================================================================================================================ DAS plans
def _half_round(x):
    return x.real.astype(np.float16).astype(np.float64) + 1j * x.imag.astype(np.float16).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _das_case(seq, interp):
    return make_case(seq=seq, interp=interp, seed=7, N=16, M=7 if seq == "PW" else None, I1=37, I2=5)     # 185 pixels: partial pixel tiles both ways


@functools.lru_cache(maxsize=None)
def _das_ref(seq, interp, fun, prec):
    from oracle import das_oracle as O
    case = _das_case(seq, interp)
    x = _half_round(case["x"]) if prec == "halfT" else case["x"]
    c = case["c"] if prec == "double" else cinv_f32(case["c"])          # (tests/test_gpu_parity.py: run_oracle / _oracle64)
    ref = O.das_spec(fun, case["Pi"], case["Pr"], case["Pv"], case["Nv"], x, case["t0"], case["fs"], c, VS=case["VS"], DV=case["DV"], interp=interp)
    ref.setflags(write=False)
    return ref


def _das_tol(interp, kernel, prec, fun):
    """the bounds of tests/test_gpu_parity.py: tol_for (fp32 'DAS'), TOL32 (test_keep_modes), 2e-3 (test_half_precision), 1e-10 (fp64)"""
    from tests.test_gpu_parity import TOL32, tol_for
    if prec == "double":
        return 1e-10
    t = tol_for(interp, kernel) if fun == "DAS" else max(TOL32, tol_for(interp, kernel))
    return max(t, 2e-3) if prec == "halfT" else t


def _das_plan(seq, interp, fun, prec, kernel, **kw):
    from qups_amd import DasPlan, build_problem, parse_options
    from qups_amd.das_spec import _cast_data, _colmajor
    case = _das_case(seq, interp)
    xt = torch.from_numpy(case["x"])
    po = parse_options(xt, list(case["opt"]) + ["interp", interp, "input-precision", prec])
    prob = build_problem(fun, case["Pi"], case["Pr"], case["Pv"], case["Nv"], tuple(xt.shape), case["t0"], case["fs"], case["c"], po)
    plan = DasPlan(prob, kernel=kernel, **kw)
    xc = _colmajor(_cast_data(xt, prec, plan.device))
    return plan, xc.reshape(1, *xc.shape)


def _planes(y, ref):
    """(1, oM, oN, count) device output and the oracle's I1 x I2 x 1 x N' x M' -> count x planes, both"""
    P = ref.shape[3] * ref.shape[4]
    return _np(y).reshape(P, -1).T, ref.reshape(-1, P, order="F")


@entry("das_plan")
@pytest.mark.parametrize("interp", ["nearest", "lanczos3"])
@pytest.mark.parametrize("kernel", [2, 1], ids=["tiled", "generic"])
@pytest.mark.parametrize("prec", ["single", "halfT", "double"])
@pytest.mark.parametrize("seq", ["FSA", "PW"])
def test_das_plan_outputs(seq, prec, kernel, interp, monkeypatch):
    """summed, keep_rx ('SYN') and keep_tx ('MUL'); the tiled kernel also without the reciprocity fold and without the lateral mirror"""
    from qups_amd import _lib
    for fun in ("DAS", "SYN", "MUL"):
        modes = [{}] if (kernel == 1 or fun != "DAS") else [{}, dict(fold=False), dict(mirror=False), dict(fold=False, mirror=False)]
        for kw in modes:
            try:
                plan, xc = _das_plan(seq, interp, fun, prec, kernel, **kw)
            except _lib.QdasError as e:                           # the one combination the library refuses: a kept dimension of fp16 / fp64 data on the tiled kernel
                assert kernel == 2 and fun != "DAS" and prec != "single" and "tiled kernel needs the 'DAS' mode (or fp32 data" in str(e), (fun, prec, str(e))
                continue
            with plan:
                assert plan.kernel == ("tiled" if kernel == 2 else "generic")
                y = guarded("das_plan", lambda: plan.execute_colmajor(xc, 1), monkeypatch)
                got, ref = _planes(y, _das_ref(seq, interp, fun, prec))
                err = rel_err(got, ref)
                print(f"das_plan {seq} {prec} {plan.kernel} {interp} {fun} {kw}: rel_err={err:.3e}")
                assert err <= _das_tol(interp, kernel, prec, fun), (fun, kw, err)


@entry("das_plan_slab")
@pytest.mark.parametrize("kernel", [2, 1], ids=["tiled", "generic"])
@pytest.mark.parametrize("seq", ["FSA", "PW"])
def test_das_plan_slab_into_a_larger_image_leaves_its_neighbours_alone(seq, kernel, monkeypatch):
    """pixels [50, 127) of 185 (neither end on a tile edge) through execute_into, into the middle of a full-size image that starts as the sentinel"""
    b, n, I = 50, 77, 185
    plan, xc = _das_plan(seq, "lanczos3", "DAS", "single", kernel, i_begin=b, i_count=n)
    with plan:
        plan.execute_colmajor(xc, 1)
        torch.cuda.synchronize()
        with GD.guard_outputs(monkeypatch) as g:
            big = torch.empty((I,), dtype=torch.complex64, device=plan.device)
            plan.execute_into(xc, big[b:b + n].reshape(1, 1, 1, n), 1)
            g.check()                                             # the bands
            raw = bits(big)
            assert bool((raw[:2 * b] == -1).all()) and bool((raw[2 * (b + n):] == -1).all()), "the slab's neighbours were written"
            assert not bool((raw[2 * b:2 * (b + n)] == -1).any()), "part of the slab was not written"
        _count("das_plan_slab", g)
        ref = _das_ref(seq, "lanczos3", "DAS", "single").reshape(-1, order="F")[b:b + n]
        assert rel_err(_np(big[b:b + n]), ref) <= _das_tol("lanczos3", kernel, "single", "DAS")


@entry("das_plan_delays")
@pytest.mark.parametrize("prec", ["single", "double"])
def test_das_plan_delays(prec, monkeypatch):
    """tests/test_gpu_parity.py test_delays: 1e-6 of the largest delay"""
    from oracle import das_oracle as O
    case = _das_case("PW", "lanczos3")
    plan, _ = _das_plan("PW", "lanczos3", "DAS", prec, 0)
    with plan:
        tau = guarded("das_plan_delays", plan.delays, monkeypatch)
    ref = O.das_spec("delays", case["Pi"], case["Pr"], case["Pv"], case["Nv"], None, 0, 1, cinv_f32(case["c"]), VS=case["VS"], DV=case["DV"])
    got = _np(tau).reshape(ref.shape, order="F")
    assert np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max()


# ================================================================================================================ das_lut, wsinterpd, shift_sum
def _lut_case():
    from oracle import das_oracle as O
    case = make_case(seq="FSA", interp="cubic", seed=21, N=6, I1=40, I2=5)          # tests/test_gpu_golden.py test_das_lut_matches_oracle
    dv, dr = O.tx_rx_distances(case["Pi"], case["Pr"], case["Pv"], case["Nv"], True, True)
    c = cinv_f32(case["c"])
    return case, dr[:, :, :, :, 0] / c, dv[:, :, :, 0, :] / c


@entry("das_lut")
@pytest.mark.parametrize("keep", [(False, False), (True, False), (False, True), (True, True)])
def test_das_lut_outputs(keep, monkeypatch):
    from oracle import das_oracle as O
    from qups_amd import sample2sep
    case, tau_rx, tau_tx = _lut_case()
    keep_rx, keep_tx = keep
    ref = O.das_lut(case["x"], tau_rx, tau_tx, case["t0"], case["fs"], interp="cubic", keep_rx=keep_rx, keep_tx=keep_tx)
    sd = (set() if keep_rx else {"rx"}) | (set() if keep_tx else {"tx"})
    for prec, tol in (("double", 1e-9), ("single", 5e-4)):
        y = guarded("das_lut", lambda: sample2sep(torch.from_numpy(case["x"]), case["t0"], case["fs"], tau_rx, tau_tx, "cubic", None, sd, 0.0, prec=prec), monkeypatch)
        assert _np(y).shape == ref.shape and rel_err(_np(y), ref) <= tol


def _ws_case(prec, M, wkind, T=300, N=5):
    """tests/test_wsinterpd.py test_wsinterpd_torch_order_record_summed_over_its_fastest_dimension"""
    rng = np.random.default_rng(19)
    dbl = prec == "double"
    ct = np.complex128 if dbl else np.complex64
    x = (rng.standard_normal((T, N, M)) + 1j * rng.standard_normal((T, N, M))).astype(ct)
    t = (np.arange(-3, T + 2, 2.5).reshape(-1, 1, 1) + rng.uniform(0, 3, (1, 1, M))).astype(np.float64 if dbl else np.float32)
    t[4, 0, M // 2] = np.inf
    w = None if wkind == "none" else rng.random((1, N, M)) + (1j * rng.random((1, N, M)) if wkind == "complex" else 0)
    if prec == "halfT":
        x = (x.real.astype(np.float16).astype(np.float32) + 1j * x.imag.astype(np.float16).astype(np.float32)).astype(np.complex64)
    wa = 1 if w is None else torch.from_numpy(w.astype(ct if wkind == "complex" else (np.float64 if dbl else np.float32)))
    return x, t, w, wa


@entry("wsinterpd")
@pytest.mark.parametrize("prec", ["single", "double", "halfT"])
@pytest.mark.parametrize("M,ev", [(33, np.nan), (31, 0.0), (12, 0.0)])
def test_wsinterpd_outputs(prec, M, ev, monkeypatch):
    from oracle import das_oracle as O
    from qups_amd.interpd import wsinterpd
    x, t, w, wa = _ws_case(prec, M, "real")
    tol = 1e-11 if prec == "double" else (2e-3 if prec == "halfT" else 3e-5)
    for terp in ("nearest", "lanczos3"):
        for sdim in ([3], None):                                  # the lane-sum kernel, and one output per lane with nothing summed
            ref = O.wsinterpd(x.astype(np.complex128), t.astype(np.float64), 1, w, sdim, terp, ev, 0.13j)
            y = guarded("wsinterpd", lambda: wsinterpd(torch.from_numpy(x), torch.from_numpy(t), 1, wa, sdim, terp, ev, 0.13j, prec=prec), monkeypatch)
            y = _np(y)
            assert y.shape == ref.shape and np.array_equal(np.isnan(y), np.isnan(ref))
            err = np.nanmax(np.abs(y - ref)) / max(1.0, np.nanmax(np.abs(ref)))
            print(f"wsinterpd {prec} M={M} {terp} sdim={sdim}: err={err:.3e} (bound {tol:g})")
            assert np.nanmax(np.abs(y - ref)) <= tol * max(1.0, np.nanmax(np.abs(ref))), (terp, sdim)


def _shift_case(dtype):
    rng = np.random.default_rng(31)
    T, N, M, Mo, pad = 300, 2, 7, 9, 40
    cplx = dtype.startswith("complex")
    x = (rng.standard_normal((T, N, M)) + (1j * rng.standard_normal((T, N, M)) if cplx else 0)).astype(dtype)
    shift = rng.uniform(-60, 60, (M, Mo))
    shift[0, 0], shift[1, 1], shift[2, 2] = -800.0, 800.0, 2.5
    w = rng.uniform(0.2, 1, (M, Mo)) * (1 + (0.5j if cplx else 0))
    w[rng.random((M, Mo)) < 0.3] = 0
    if dtype in ("complex64", "float32"):
        shift = shift.astype(np.float32).astype(np.float64)
    return x, shift, w, pad


@entry("shift_sum")
@pytest.mark.parametrize("dtype", ["complex64", "complex128", "float32", "float64"])
def test_shift_sum_outputs(dtype, monkeypatch):
    """To shorter than the padded length with tpad > 0, To past it, and no tail; tests/test_wsinterpd.py's oracle on the zero-padded record"""
    from qups_amd.interpd import shift_sum
    from tests.test_wsinterpd import _shift_ref
    x, shift, w, pad = _shift_case(dtype)
    T = x.shape[0]
    xp = np.concatenate([x, np.zeros((pad,) + x.shape[1:], x.dtype)], 0)
    tol = 1e-11 if dtype in ("complex128", "float64") else 2e-5
    for To, tpad in ((T + 17, pad), (T + pad + 30, pad), (T - 43, 0)):
        y = guarded("shift_sum", lambda: shift_sum(torch.from_numpy(x), shift, w, "cubic", To=To, tpad=tpad), monkeypatch)
        ref = _shift_ref(xp if tpad else x, shift, w, "cubic", To)
        assert tuple(y.shape) == ref.shape and rel_err(_np(y), ref) <= tol, (To, tpad)


# ================================================================================================================ convd, iir
@entry("convd")
@pytest.mark.parametrize("dtype", ["complex64", "float32", "complex128", "float64"])
@pytest.mark.parametrize("sz_x,sz_y,dim", [((301, 70), (37, 70), 1), ((3, 129, 5), (1, 9, 1), 2), ((5, 260, 70), (5, 9, 70), 2)])
def test_convd_outputs(sz_x, sz_y, dim, dtype, monkeypatch):
    """trace counts that are no multiple of 64, lengths that are no multiple of 32, the filter along either dimension; bounds of tests/test_convd.py"""
    from oracle import convd_oracle as O
    from qups_amd import convd
    from tests.test_convd import rel
    rng = np.random.default_rng(5)
    cplx = dtype.startswith("complex")
    x = (rng.standard_normal(sz_x) + (1j * rng.standard_normal(sz_x) if cplx else 0)).astype(dtype)
    y = (rng.standard_normal(sz_y) + (1j * rng.standard_normal(sz_y) if cplx else 0)).astype(dtype)
    tol = 2e-5 if dtype in ("complex64", "float32") else 1e4 * np.finfo(np.float64).eps
    for shape in ("full", "same", "valid"):
        ref, _ = O.convd(x, y, dim, shape)
        z = guarded("convd", lambda: convd(torch.from_numpy(x), torch.from_numpy(y), dim, shape), monkeypatch)
        assert tuple(z.shape) == ref.shape and rel(_np(z), ref) <= tol, shape


@entry("iir")
@pytest.mark.parametrize("dtype,cplx", [("float32", True), ("float32", False), ("float64", True), ("float64", False)])
def test_sosfilt_outputs(dtype, cplx, monkeypatch):
    """tests/test_convd.py test_sosfilt_on_the_device"""
    from scipy import signal
    from oracle import convd_oracle as O
    from qups_amd import sosfilt
    from tests.test_convd import rel
    rng = np.random.default_rng(7)
    for shape, dim, sos, gain in (((301, 70), 1, signal.butter(4, [0.1, 0.4], "band", output="sos"), 1.0),
                                  ((3, 129, 5), 2, signal.cheby1(5, 1.0, 0.3, output="sos"), 0.5),
                                  ((33, 1), 1, np.array([[0.5, 0.25, 0.0, 2.0, -0.6, 0.0]]), 3.0)):
        x = rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if cplx else 0)
        x = x.astype({"float32": np.complex64 if cplx else np.float32, "float64": np.complex128 if cplx else np.float64}[dtype])
        y = guarded("iir", lambda: sosfilt(torch.from_numpy(x), sos, dim, gain), monkeypatch)
        ref = O.sosfilt(x.astype(np.complex128 if cplx else np.float64), sos, dim - 1, gain)
        assert tuple(y.shape) == x.shape and rel(_np(y), ref) <= (1e-6 if dtype == "float32" else 1e-13), (shape, dim)


# ================================================================================================================ hilbert / downmix
@entry("hilbert")
@pytest.mark.parametrize("force_hipfft", [False, True])
@pytest.mark.parametrize("T,N,K,dtype,fdown", [(301, None, 3, "f32", 0.0), (300, 512, 5, "f32", 0.0), (2816, None, 7, "f32", 0.0),
                                               (400, 256, 5, "i16", 0.0), (384, 512, 3, "i16", 4.0e6)])
def test_hilbert_outputs(T, N, K, dtype, fdown, force_hipfft, monkeypatch):
    """tests/test_preproc.py: 2e-5 of the peak against the numpy restatement"""
    from qups_amd.preproc import hilbert
    from tests.test_preproc import hilbert_ref
    monkeypatch.setenv("QDAS_PRE_HIPFFT", "1" if force_hipfft else "0")
    rng = np.random.default_rng(T + K)
    x = rng.standard_normal((T, K))
    fs, t0 = 20e6, 1.7e-6
    xq = np.round(x * 3000).astype(np.int16) if dtype == "i16" else x.astype(np.float32)
    ref = hilbert_ref(xq.astype(np.float64), N, fdown, t0, fs)
    y = guarded("hilbert", lambda: hilbert(xq, N, fdown, t0, fs), monkeypatch)
    assert hilbert.last_one_pass == (not force_hipfft and T != 301)          # 301 = 7 x 43: not a length of the one-pass kernel
    y = y.cpu().numpy()
    assert y.shape == ref.shape and np.abs(y - ref).max() / np.abs(ref).max() <= 2e-5


# ================================================================================================================ greens
@entry("greens")
@pytest.mark.parametrize("prec", ["single", "double"])
def test_greens_outputs(prec, monkeypatch):
    """the smallest case of tests/test_greens.py (40 scatterers, 2 x 3 sub-elements), its bounds"""
    from oracle import greens_oracle as GO
    from qups_amd.greens import greens_kernel
    from tests.test_greens import _setup
    g = _setup(seed=5, N=9, M=7, I=40, En=2, Em=3, fsr=1.0)
    args = (g["Ps"], g["a"], g["Pr"], g["Pv"], g["x"], g["S"], g["s0"], g["t0"], g["fs"], 1.0, g["cinv"], g["R0"], "linear")
    ref = GO.greens_kernel(*args)
    y = guarded("greens", lambda: greens_kernel(*args, prec), monkeypatch)
    out = _np(y)
    assert out.shape == ref.shape and np.abs(out - ref).max() / np.abs(ref).max() <= (1e-10 if prec == "double" else 3e-4)


# ================================================================================================================ permute3
@entry("permute3")
@pytest.mark.parametrize("dtype", ["float16", "float32", "complex64", "complex128"])
def test_permute3_outputs(dtype, monkeypatch):
    """65 x 3 x 33: one past a 64-row tile, a ragged 33; element sizes 2, 4, 8 and 16 (tests/test_gpu_edges.py test_colmajor_layout_kernel: equality)"""
    from qups_amd.das_spec import _colmajor
    gen = torch.Generator(device="cuda").manual_seed(101)
    shape = (65, 3, 33)
    t = torch.randn(shape + ((2,) if dtype.startswith("complex") else ()), generator=gen, device="cuda", dtype=torch.float64 if dtype == "complex128" else torch.float32)
    t = (torch.view_as_complex(t) if dtype.startswith("complex") else t.to(getattr(torch, dtype))).contiguous()
    out = guarded("permute3", lambda: _colmajor(t), monkeypatch)
    assert out.is_contiguous() and same_bits(out, t.permute(2, 1, 0).contiguous())


# ================================================================================================================ coherence
@entry("coherence")
@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("method,cplx", [(m, c) for m in ["average", "ensemble", "dmas", "cohfac", "pcf"] for c in (True, False) if m != "pcf" or c])
def test_coherence_outputs(method, cplx, f64, monkeypatch):
    """N = 7, 111 pixels, every second row of a wider buffer; tests/test_gpu_coherence.py's restatement and bounds"""
    from tests import test_gpu_coherence as H
    x = H._data((37, 3, 7), cplx, seed=sum(map(ord, f"{method}{f64}{cplx}")), zero_px=True)
    dt = {(False, False): torch.float32, (False, True): torch.complex64, (True, False): torch.float64, (True, True): torch.complex128}[(f64, cplx)]
    xt = H._layout(x, dt, "odd")
    y = guarded("coherence", lambda: H._run(method, xt, 3), monkeypatch)
    H._check(method, y, _np(xt).astype(np.complex128 if cplx else np.float64), 2, f64=f64)


# ================================================================================================================ eikonal
@entry("eikonal")
@pytest.mark.parametrize("shape", [(3, 3), (17, 33)])
def test_eikonal_outputs(shape, monkeypatch):
    from tests import eikonal_ref as R
    from tests import test_gpu_eikonal as H
    C1, C2 = shape
    c = R.smooth_random(C1, C2, seed=C1 + 100 * C2)
    sets = [[[1.0], [1.0]], [[C1], [C2]], [[min((C1 + 1) / 2 + 0.25, C1)], [min((C2 + 1) / 2 + 0.25, C2)]]]
    T = guarded("eikonal", lambda: H._solve(c, H.DP, sets), monkeypatch)
    H._check_maps(c, H.DP, sets, T)


@entry("eikonal_tables")
def test_eikonal_tables_into_a_slab_of_a_larger_buffer(monkeypatch):
    """``out=`` rows [2, 5) of a 7-row table: the rows around them keep the sentinel; pixels off the grid are NaN (tests/test_gpu_eikonal.py's table bound)"""
    from qups_amd import eikonal as E
    from tests import eikonal_ref as R
    from tests import test_gpu_eikonal as H
    C1, C2, K = 17, 33, 3
    c = R.smooth_random(C1, C2, seed=C1 + 100 * C2)
    src = np.array([[1.0, 9.3, 17.0], [1.0, 20.1, 33.0]])
    T = H._solve(c, H.DP, [src[:, k:k + 1] for k in range(K)])
    rng = np.random.default_rng(3)
    Pi = np.stack([rng.uniform(0.2, C1 + 0.8, 75), rng.uniform(0.2, C2 + 0.8, 75)])          # 75 pixels, some outside the grid
    E.eikonal_tables(T, Pi)
    torch.cuda.synchronize()
    with GD.guard_outputs(monkeypatch) as g:
        buf = torch.empty((K + 4, 75), dtype=torch.float64, device="cuda")
        tau = E.eikonal_tables(T, Pi, out=buf[2:2 + K])
        g.check()
        raw = bits(buf)
        assert bool((raw[:2] == -1).all()) and bool((raw[2 + K:] == -1).all()), "rows outside the slab were written"
        assert not bool((raw[2:2 + K] == -1).any()), "part of the slab was not written"
    _count("eikonal_tables", g)
    a = _np(tau)
    ref = np.stack([R.sample(R.fmm(c, H.DP, src[:, k:k + 1]), Pi) for k in range(K)], -1)
    assert a.shape == ref.shape and np.array_equal(np.isnan(a), np.isnan(ref)) and np.isnan(a).any() and not np.isnan(a).all()
    ok = ~np.isnan(ref)
    assert np.all(np.abs(a[ok] - ref[ok]) <= 1e-9 * H.DP / c.max() + 1e-12 * np.abs(ref[ok]))
    # the same through the fresh allocations of eikonal_tables and travel_time_tables (sources in blocks of two maps)
    tau2 = guarded("eikonal_tables", lambda: E.eikonal_tables(T, Pi), monkeypatch)
    assert np.array_equal(_np(tau2), a, equal_nan=True)
    tt = guarded("eikonal_tables", lambda: E.travel_time_tables(c, H.DP, src, Pi, (75, 1, 1), budget=2 * C1 * C2 * 8), monkeypatch)
    assert np.array_equal(_np(tt).reshape(75, K), a, equal_nan=True)


# ================================================================================================================ adjoint
@pytest.fixture(scope="module")
def adj_core():
    from tests import test_gpu_adjoint as H
    us = H._system("PW", 20, 7, 37, 5)
    x, t0 = H._data(96, 20, 7, seed=1)
    return us, x, t0


# bfAdjoint stacks its frames (a copy in torch), so the result does not alias the buffer qdas_adjoint filled -- the only one the call takes from torch.empty:
# every guarded buffer must be fully written instead
ADJ = dict(require=False, all_written=True)


@entry("adjoint")
@pytest.mark.parametrize("keep_rx,keep_tx", [(False, False), (False, True), (True, False), (True, True)])
def test_adjoint_outputs(adj_core, keep_rx, keep_tx, monkeypatch):
    """the core shape of tests/test_gpu_adjoint.py (PW, N = 20, V = 7, 37 x 5 pixels, T = 96) in the four output modes, whole and in pixel blocks"""
    from tests import test_gpu_adjoint as H
    us, x, t0 = adj_core
    ref, _ = H._oracle(us, x, t0, fmod=2.5e6, keep_rx=keep_rx, keep_tx=keep_tx)
    for block in (None, "20000"):
        if block:
            monkeypatch.setenv("QDAS_ADJOINT_BLOCK_BYTES", block)
        b = guarded("adjoint", lambda: H._run(us, x, t0, fmod=2.5e6, keep_rx=keep_rx, keep_tx=keep_tx), monkeypatch, **ADJ)
        assert H._err(torch.from_numpy(H._flat(b, us)), ref, f"guarded keep_rx={keep_rx} keep_tx={keep_tx} block={block}") <= H.TOL


@entry("adjoint")
def test_adjoint_outputs_two_transmit_groups_kept(monkeypatch):
    """V = 70 with keep_tx: the second group of transmits holds 6"""
    from tests import test_gpu_adjoint as H
    us = H._system("PW", 20, 70, 9, 5)
    x, t0 = H._data(48, 20, 70, seed=3)
    ref, _ = H._oracle(us, x, t0, keep_tx=True)
    b = guarded("adjoint", lambda: H._run(us, x, t0, keep_tx=True), monkeypatch, **ADJ)
    assert H._err(torch.from_numpy(H._flat(b, us)), ref, "guarded PW V=70 keep_tx") <= H.TOL


# ================================================================================================================ migration
@entry("migration")
@pytest.mark.parametrize("kw", [dict(), dict(keep_tx=True), dict(frames=2), dict(frames=2, keep_tx=True)], ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()) or "summed")
@pytest.mark.parametrize("which", [1, 4], ids=["padded", "truncated"])
def test_migration_outputs(which, kw, monkeypatch):
    from qups_amd import migration as MG
    from tests import test_gpu_migration as H
    T, N, M, nfft = shape = H.SHAPES[which]
    x, tau, gam = H._data(T, N, M, kw.get("frames", 1))
    xd = torch.from_numpy(x).cuda()
    b = guarded("migration", lambda: MG.migrate(xd, H.T0, H.FS, tau, gam, H.PITCH, H.C0, nfft, 0.0, "cubic", True, kw.get("keep_tx", False)), monkeypatch)
    assert H._err(b, H._ref(T, N, M, nfft, "cubic", True, kw.get("keep_tx", False), 0.0, kw.get("frames", 1)), f"guarded {shape} {kw}") <= H.BOUND_FUSED


@entry("migration")
@pytest.mark.parametrize("per_block,fill", [(2, 1), (4, None), (4, 32), (1, None)])
def test_migration_outputs_transmit_blocks_and_slices(per_block, fill, monkeypatch):
    from qups_amd import migration as MG
    from tests import test_gpu_migration as H
    T, N, M, nfft = 64, 16, 5, None
    monkeypatch.setenv("QDAS_MIGRATION_BLOCK_BYTES", str(per_block * 64 * 16 * 8))
    if fill is not None:
        monkeypatch.setenv("QDAS_MIGRATION_FILL", str(fill))
    x, tau, gam = H._data(T, N, M)
    xd = torch.from_numpy(x).cuda()
    for keep_tx in (False, True):
        b = guarded("migration", lambda: MG.migrate(xd, H.T0, H.FS, tau, gam, H.PITCH, H.C0, nfft, 0.0, "cubic", True, keep_tx), monkeypatch)
        assert H._err(b, H._ref(T, N, M, nfft, "cubic", True, keep_tx), f"guarded blocks {per_block} {fill} keep_tx={keep_tx}") <= H.BOUND_FUSED


@entry("migration_compose")
def test_migration_compose_outputs(monkeypatch):
    """the length with a radix of 17: torch's FFTs around wsinterpd.  The result comes out of torch operations, so only the bands of what the wrappers allocate are checked"""
    from qups_amd import migration as MG
    from tests import test_gpu_migration as H
    T, N, M, nfft = H.ODD
    x, tau, gam = H._data(T, N, M)
    xd = torch.from_numpy(x).cuda()
    b = guarded("migration_compose", lambda: MG.compose(xd, H.T0, H.FS, tau, gam, H.PITCH, H.C0, nfft), monkeypatch, require=False)
    assert H._err(b, H._ref(T, N, M, nfft), "guarded compose 34x12") <= H.BOUND_COMPOSE


# ================================================================================================================ poisoned halos
@entry("halo")
@pytest.mark.parametrize("kernel", [2, 1], ids=["tiled", "generic"])
@pytest.mark.parametrize("prec", ["single", "halfT"])
def test_halo_das_short_record(prec, kernel):
    """T = 300 against a 30 mm path (tests/test_gpu_parity.py test_edges_and_out_of_record): windows hang over both ends of the traces.  Plans are bit-reproducible
    (test_frames_and_plan_reuse)."""
    from oracle import das_oracle as O
    from qups_amd import DasPlan, build_problem, parse_options
    from qups_amd.das_spec import _cast_data, _colmajor
    case = make_case(seq="FSA", interp="lanczos3", seed=14, T=300, data="noise", zlim=(1e-3, 30e-3), I1=37, I2=5, N=16)
    xt = torch.from_numpy(case["x"])
    po = parse_options(xt, list(case["opt"]) + ["interp", "lanczos3", "input-precision", prec])
    prob = build_problem("DAS", case["Pi"], case["Pr"], case["Pv"], case["Nv"], tuple(xt.shape), case["t0"], case["fs"], case["c"], po)
    with DasPlan(prob, kernel=kernel) as plan:
        xc = _colmajor(_cast_data(xt, prec, plan.device))
        y = halo_runs(lambda xh: plan.execute_colmajor(xh.reshape(1, *xh.shape), 1), [xc])
    x = _half_round(case["x"]) if prec == "halfT" else case["x"]
    ref = O.das_spec("DAS", case["Pi"], case["Pr"], case["Pv"], case["Nv"], x, case["t0"], case["fs"], cinv_f32(case["c"]), VS=case["VS"], DV=case["DV"], interp="lanczos3")
    tol = 2e-3 if prec == "halfT" else (3e-4 if kernel == 1 else 3e-5)          # (test_edges_and_out_of_record; test_half_precision)
    assert rel_err(_np(y).reshape(-1), ref.reshape(-1, order="F")) <= tol


@entry("halo")
def test_halo_das_lut_and_wsinterpd():
    from oracle import das_oracle as O
    from qups_amd.interpd import das_lut, wsinterpd
    case, tau_rx, tau_tx = _lut_case()
    fs, t0 = case["fs"], case["t0"]
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)
    x, n1, n2 = dev(case["x"], torch.complex64), dev(tau_rx * fs, torch.float32), dev((tau_tx - t0) * fs, torch.float32)
    y = halo_runs(lambda xh, a, b: das_lut(xh, a, b, interp="cubic", keep_rx=True, prec="single"), [x, n1, n2])
    ref = O.das_lut(case["x"], tau_rx, tau_tx, t0, fs, interp="cubic", keep_rx=True, keep_tx=False)
    assert rel_err(_np(y).reshape(ref.shape), ref) <= 5e-4
    xs, ts, w, wa = _ws_case("single", 33, "real")
    for sdim in ([3], None):
        y = halo_runs(lambda xh, th, wh: wsinterpd(xh, th, 1, wh, sdim, "lanczos3", 0.0, 0.13j, prec="single"), [dev(xs, torch.complex64), dev(ts, torch.float32), wa.cuda()])
        ref = O.wsinterpd(xs.astype(np.complex128), ts.astype(np.float64), 1, w, sdim, "lanczos3", 0.0, 0.13j)
        assert np.nanmax(np.abs(_np(y) - ref)) <= 3e-5 * max(1.0, np.nanmax(np.abs(ref)))


@entry("halo")
@pytest.mark.parametrize("dtype", ["complex64", "float32"])
def test_halo_shift_sum(dtype):
    from qups_amd.interpd import shift_sum
    from tests.test_wsinterpd import _shift_ref
    x, shift, w, pad = _shift_case(dtype)
    T = x.shape[0]
    sh = torch.from_numpy(shift).cuda()
    wt = torch.from_numpy(w).cuda()
    y = halo_runs(lambda xh, s, ww: shift_sum(xh, s, ww, "cubic", To=T + 17, tpad=pad), [torch.from_numpy(x).cuda(), sh, wt])
    xp = np.concatenate([x, np.zeros((pad,) + x.shape[1:], x.dtype)], 0)
    assert rel_err(_np(y), _shift_ref(xp, shift, w, "cubic", T + 17)) <= 2e-5


@entry("halo")
def test_halo_convd_iir_hilbert():
    from scipy import signal
    from oracle import convd_oracle as O
    from qups_amd import convd, sosfilt
    from qups_amd.preproc import hilbert
    from tests.test_convd import rel
    from tests.test_preproc import hilbert_ref
    rng = np.random.default_rng(8)
    x = (rng.standard_normal((301, 70)) + 1j * rng.standard_normal((301, 70))).astype(np.complex64)
    k = (rng.standard_normal((37, 70)) + 1j * rng.standard_normal((37, 70))).astype(np.complex64)
    z = halo_runs(lambda a, b: convd(a, b, 1, "same"), [torch.from_numpy(x).cuda(), torch.from_numpy(k).cuda()])
    assert rel(_np(z), O.convd(x, k, 1, "same")[0]) <= 2e-5
    sos = signal.butter(4, [0.1, 0.4], "band", output="sos")
    z = halo_runs(lambda a: sosfilt(a, sos, 1, 1.0), [torch.from_numpy(x).cuda()])
    assert rel(_np(z), O.sosfilt(x.astype(np.complex128), sos, 0, 1.0)) <= 1e-6
    for T, N, dt in ((300, 512, np.float32), (301, None, np.float32), (400, 256, np.int16)):
        xr = rng.standard_normal((T, 5))
        xq = np.round(xr * 3000).astype(np.int16) if dt == np.int16 else xr.astype(np.float32)
        z = halo_runs(lambda a: hilbert(a, N), [torch.from_numpy(xq).cuda()])
        ref = hilbert_ref(xq.astype(np.float64), N)
        assert np.abs(_np(z) - ref).max() / np.abs(ref).max() <= 2e-5


@entry("halo")
def test_halo_coherence_permute3_and_eikonal():
    from qups_amd.das_spec import _colmajor
    from tests import eikonal_ref as R
    from tests import test_gpu_coherence as H
    from tests import test_gpu_eikonal as HE
    x = H._data((37, 3, 7), True, seed=4, zero_px=True)
    xt = H._layout(x, torch.complex64, "odd")                       # a strided view: the skipped rows are poisoned too
    for method in H.METHODS:
        y = halo_runs(lambda a: H._run(method, a, 3), [xt])
        H._check(method, y, _np(xt), 2)
    t = torch.randn((65, 3, 33), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    assert same_bits(halo_runs(_colmajor, [t]), t.permute(2, 1, 0).contiguous())
    c = R.smooth_random(17, 33, seed=17 + 3300)
    sets = [[[1.0], [1.0]], [[17.0], [33.0]]]
    T = halo_runs(lambda cc: HE._solve(cc, HE.DP, sets).contiguous(), [torch.from_numpy(c).cuda()])
    HE._check_maps(c, HE.DP, sets, T)


@entry("halo")
def test_halo_eikonal_tables():
    """the sampler reads the maps where they lie (a C1 x C2 x K view of K x C2 x C1 storage is taken without a copy): cubic stencils at the rim of the grid and
    pixels off the grid, with the maps and the pixel coordinates haloed"""
    from qups_amd import eikonal as E
    from tests import eikonal_ref as R
    from tests import test_gpu_eikonal as H
    C1, C2, K = 17, 33, 3
    c = R.smooth_random(C1, C2, seed=C1 + 100 * C2)
    src = np.array([[1.0, 9.3, 17.0], [1.0, 20.1, 33.0]])
    Tm = H._solve(c, H.DP, [src[:, k:k + 1] for k in range(K)]).permute(2, 1, 0)
    assert Tm.is_contiguous() and tuple(Tm.shape) == (K, C2, C1)
    rng = np.random.default_rng(3)
    Pi = np.stack([rng.uniform(0.2, C1 + 0.8, 75), rng.uniform(0.2, C2 + 0.8, 75)])
    Pi[:, :4] = [[1.0, C1, 1.0, C1], [1.0, 1.0, C2, C2]]                          # the four corner nodes themselves
    tau = halo_runs(lambda Th, Ph: E.eikonal_tables(Th.permute(2, 1, 0), Ph).contiguous(), [Tm, torch.from_numpy(Pi).cuda()])
    a = _np(tau)
    ref = np.stack([R.sample(R.fmm(c, H.DP, src[:, k:k + 1]), Pi) for k in range(K)], -1)
    assert a.shape == ref.shape and np.array_equal(np.isnan(a), np.isnan(ref)) and np.isnan(a).any() and not np.isnan(a[:4]).any()
    ok = ~np.isnan(ref)
    assert np.all(np.abs(a[ok] - ref[ok]) <= 1e-9 * H.DP / c.max() + 1e-12 * np.abs(ref[ok]))          # (tests/test_gpu_eikonal.py's table bound)


@entry("halo")
def test_halo_migration_and_adjoint(adj_core):
    from qups_amd import ChannelData
    from qups_amd import migration as MG
    from tests import test_gpu_adjoint as HA
    from tests import test_gpu_migration as H
    T, N, M, nfft = H.SHAPES[1]
    x, tau, gam = H._data(T, N, M)
    b = halo_runs(lambda xh: MG.migrate(xh, H.T0, H.FS, tau, gam, H.PITCH, H.C0, nfft), [torch.from_numpy(x).cuda()])
    assert H._err(b, H._ref(T, N, M, nfft), "halo padded") <= H.BOUND_FUSED
    T, N, M, nfft = H.SHAPES[0]                                     # the strided view of test_fused_noncontiguous_view
    x, tau, gam = H._data(T, N, M)
    big = torch.zeros((2 * T, N + 3, M, 1), dtype=torch.complex64, device="cuda")
    big[::2, 1:N + 1] = torch.from_numpy(x).cuda()
    b = halo_runs(lambda xh: MG.migrate(xh, H.T0, H.FS, tau, gam, H.PITCH, H.C0), [big[::2, 1:N + 1]])
    assert H._err(b, H._ref(T, N, M, nfft), "halo view") <= H.BOUND_FUSED
    us, xa, t0 = adj_core
    ref, _ = HA._oracle(us, xa, t0, fmod=2.5e6)
    b = halo_runs(lambda xh: us.bfAdjoint(ChannelData(xh, t0, HA.FS), fmod=2.5e6), [torch.from_numpy(xa).cuda()])
    assert HA._err(torch.from_numpy(HA._flat(b, us)), ref, "halo core") <= HA.TOL


# ================================================================================================================ isolation between traces
POISON = (float("nan"), float("inf"))


def _poisoned(x, idx, value, part):
    """x (T first) with trace ``idx`` replaced by ``value``: all of it, or its first and last 8 samples -- the ones a neighbour's window overhangs"""
    xp = x.clone()
    v = complex(value, value) if x.is_complex() else value
    if part == "whole":
        xp[(slice(None),) + idx] = v
    else:
        xp[(slice(0, 8),) + idx] = v
        xp[(slice(-8, None),) + idx] = v
    return xp


def _others_equal(a, b, drop, what):
    """every slice of the two results but ``drop`` (an index tuple with slices) is bit-identical, and finite"""
    mask = torch.ones(a.shape, dtype=torch.bool, device=a.device)
    mask[drop] = False
    ra, rb = (torch.view_as_real(t) if t.is_complex() else t for t in (a, b))
    m = mask.unsqueeze(-1).expand(ra.shape) if a.is_complex() else mask
    assert bool(torch.isfinite(ra[m]).all()), f"{what}: a non-finite value outside the poisoned slice"
    assert bool(torch.equal(bits(ra[m]), bits(rb[m]))), f"{what}: slices other than the poisoned one changed"


@entry("isolation")
@pytest.mark.parametrize("kernel", [2, 1], ids=["tiled", "generic"])
@pytest.mark.parametrize("prec", ["single", "halfT"])
def test_isolation_das_kept_dimensions(prec, kernel):
    """'BF' (both dimensions kept): a NaN / Inf trace (n*, m*) changes plane (n*, m*) only"""
    from qups_amd import _lib, das_spec
    case = make_case(seq="PW", interp="lanczos3", seed=9, N=16, M=7, I1=37, I2=5, data="noise")
    N, M = case["N"], case["M"]

    def run(x):
        y = das_spec("BF", case["Pi"], case["Pr"], case["Pv"], case["Nv"], x, case["t0"], case["fs"], case["c"], *case["opt"],
                     "interp", "lanczos3", "input-precision", prec, kernel=kernel, return_plan=True)
        y, plan = y
        torch.cuda.synchronize()
        assert plan.kernel == ("tiled" if kernel == 2 else "generic"), plan.kernel_name()
        return y.to(torch.complex64)                              # (exact for fp16 results; complex32 has few operators)
    x = torch.from_numpy(case["x"]).cuda()
    try:
        clean = run(x)
    except _lib.QdasError as e:
        assert kernel == 2 and prec == "halfT" and "tiled kernel needs the 'DAS' mode (or fp32 data" in str(e), str(e)
        pytest.skip("the library refuses fp16 data with kept dimensions on the tiled kernel: " + str(e))
    assert tuple(clean.shape[:5]) == (37, 5, 1, N, M) and bool(torch.isfinite(torch.view_as_real(clean)).all())
    for n, m in ((5, 3), (0, 0), (N - 1, M - 1)):
        for value in POISON:
            for part in ("whole", "ends"):
                y = run(_poisoned(x, (n, m), value, part))
                _others_equal(y, clean, (slice(None), slice(None), slice(None), n, m), f"BF {prec} kernel={kernel} trace=({n},{m}) {value} {part}")


@entry("isolation")
def test_isolation_das_lut_and_wsinterpd():
    from qups_amd.interpd import das_lut, wsinterpd
    case, tau_rx, tau_tx = _lut_case()
    fs, t0 = case["fs"], case["t0"]
    N = M = 6
    x = torch.from_numpy(case["x"]).cuda()
    n1, n2 = torch.from_numpy(tau_rx * fs).cuda(), torch.from_numpy((tau_tx - t0) * fs).cuda()
    run = lambda xx: das_lut(xx, n1, n2, interp="cubic", keep_rx=True, keep_tx=True, prec="single")
    clean = run(x)
    assert tuple(clean.shape) == (40, 5, 1, N, M)
    for n, m in ((2, 3), (0, 0), (N - 1, M - 1)):
        for value in POISON:
            for part in ("whole", "ends"):
                _others_equal(run(_poisoned(x, (n, m), value, part)), clean, (slice(None), slice(None), slice(None), n, m), f"das_lut ({n},{m}) {value} {part}")
    xs, ts, w, wa = _ws_case("single", 33, "real")
    ts = ts.copy()
    ts[4, 0, 16] = 7.0                                            # (finite delays only: every output of the clean run is finite)
    xd, td = torch.from_numpy(xs).cuda(), torch.from_numpy(ts).cuda()
    run = lambda xx: wsinterpd(xx, td, 1, wa, None, "lanczos3", 0.0, 0.13j, prec="single")
    clean = run(xd)
    assert tuple(clean.shape) == (ts.shape[0], 5, 33)
    for n, m in ((2, 16), (0, 0), (4, 32)):
        for value in POISON:
            for part in ("whole", "ends"):
                _others_equal(run(_poisoned(xd, (n, m), value, part)), clean, (slice(None), n, m), f"wsinterpd ({n},{m}) {value} {part}")


@entry("isolation")
def test_isolation_migration_and_adjoint_kept_transmits(adj_core):
    from qups_amd import ChannelData
    from qups_amd import migration as MG
    from tests import test_gpu_adjoint as HA
    from tests import test_gpu_migration as H
    T, N, M, nfft = H.SHAPES[1]
    x, tau, gam = H._data(T, N, M)
    xd = torch.from_numpy(x).cuda()
    run = lambda xx: MG.migrate(xx, H.T0, H.FS, tau, gam, H.PITCH, H.C0, nfft, 0.0, "cubic", True, True)
    clean = run(xd)
    assert clean.shape[2] == M
    for m in range(M):
        for value in POISON:
            xp = xd.clone()
            xp[:, :, m] = complex(value, value)
            _others_equal(run(xp), clean, (slice(None), slice(None), m), f"migration transmit {m} {value}")
    us, xa, t0 = adj_core
    xd = torch.from_numpy(xa).cuda()
    run = lambda xx: us.bfAdjoint(ChannelData(xx, t0, HA.FS), fmod=2.5e6, keep_tx=True)
    clean = run(xd)
    assert tuple(clean.shape) == (37, 5, 1, 1, 7)
    for v in (0, 3, 6):
        for value in POISON:
            xp = xd.clone()
            xp[:, :, v] = complex(value, value)
            _others_equal(run(xp), clean, (slice(None), slice(None), slice(None), slice(None), v), f"adjoint transmit {v} {value}")


@entry("isolation")
@pytest.mark.parametrize("method", ["average", "ensemble", "dmas", "cohfac", "pcf"])
def test_isolation_coherence_pixels(method):
    """one pixel's aperture vector NaN / Inf: every other pixel keeps its bits (tests/test_gpu_coherence.py test_nan_samples checks values, not isolation)"""
    from tests import test_gpu_coherence as H
    x = H._data((37, 3, 7), True, seed=21)
    xt = H._layout(x, torch.complex64, "das")
    both = lambda r: tuple(r) if isinstance(r, (tuple, list)) else (r,)          # (pcf returns w and sf: two outputs of the one kernel)
    clean = both(H._run(method, xt, 3))
    assert len(clean) == (2 if method == "pcf" else 1)
    for i, j in ((0, 0), (18, 1), (36, 2)):
        for value in POISON:
            xp = xt.clone()
            xp[i, j, :] = complex(value, value)
            assert xp.stride() == xt.stride()
            for k, (got, want) in enumerate(zip(both(H._run(method, xp, 3)), clean)):
                _others_equal(got, want, (i, j), f"{method} output {k} pixel ({i},{j}) {value}")


# ================================================================================================================ summary
def test_zz_every_entry_ran_at_least_one_guarded_case(request, capsys):
    """one line per entry -- cases, bytes guarded -- so that an entry whose cases were all skipped shows"""
    mine = {ENTRY_OF[i.originalname] for i in request.session.items
            if i.module.__name__ == __name__ and getattr(i, "originalname", None) in ENTRY_OF and ENTRY_OF[i.originalname] not in ("halo", "isolation")}
    lines = [f"guards: {name:18s} cases={n:4d} bytes_guarded={nb:10d} result=ok" for name, (n, nb) in SUMMARY.items()]
    lines += [f"guards: {name:18s} cases=   0 result=NOT RUN" for name in sorted(mine - set(SUMMARY))]
    with capsys.disabled():                                          # (shown without -s: the lines are the evidence that no entry was skipped)
        print("\n" + "\n".join(lines))
    if not os.environ.get("PYTEST_XDIST_WORKER"):                  # (under xdist the cases ran in other processes)
        assert not (mine - set(SUMMARY)), sorted(mine - set(SUMMARY))
