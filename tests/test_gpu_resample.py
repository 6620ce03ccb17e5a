"""qdas_resample and its Python layer (qups_amd/resample.py, ChannelData.resample / filtfilt / fftfilt) on the device, against the float64 restatement
tests/resample_ref.py and against scipy.

TOLERANCE per element (real and imaginary part separately), derived and not tuned: ``|err| <= (M + 4) eps S X`` with ``M = ceil(K / p)``,
``S = max_phi sum_m |h[phi + m p]|``, ``X = max|x|`` (``3 max|x|`` with the odd edge, whose extension reaches that) and eps = 2^-24 (2^-53 for double data):
M products and sums of one rounding each, the tap's rounding to the compute precision, the two roundings of the reflected sample, one more for slack
(tests/resample_ref.py ``bound``).  The data and the taps are random normal, so a dropped tap or a wrong phase is hundreds of bounds.  Every case prints its
own ratio err / bound as ``resample ratio``; the largest over every case of this file on one MI355X is 0.164 (K = 5 at 7/3: one tap per output, a single product beside the slack terms).

The entry takes its stream in the descriptor's ``queue`` field (the census of ``void *stream`` parameters, tests/test_streams_host.py, is a pinned list): the
stream case is in this file."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch

from qups_amd import ChannelData, DasError, Scan, Sequence, Transducer, UltrasoundSystem, _lib
from tests import guards as GD
from tests import resample_ref as R
from tests import streams as ST

pytestmark = pytest.mark.gpu

RS = importlib.import_module("qups_amd.resample")
NPT = {"i16": np.int16, "f32": np.float32, "c64": np.complex64, "f64": np.float64, "c128": np.complex128}
OUT = {"i16": torch.float32, "f32": torch.float32, "c64": torch.complex64, "f64": torch.float64, "c128": torch.complex128}
CODE = {"i16": _lib.RESAMPLE_I16, "f32": _lib.RESAMPLE_F32, "c64": _lib.RESAMPLE_C64, "f64": _lib.RESAMPLE_F64, "c128": _lib.RESAMPLE_C128}
FILL_MS = 60
SEEN = {"ratio": 0.0}


def is_double(dtname):
    return dtname in ("f64", "c128")


@functools.lru_cache(maxsize=None)
def data(T, Cn, dtname, seed=5):
    rng = np.random.default_rng(seed + 1000 * T + Cn)
    if dtname == "i16":
        x = np.clip(np.round(rng.standard_normal((T, Cn)) * 600), -2000, 2000).astype(np.int16)
    elif dtname in ("c64", "c128"):
        x = (rng.standard_normal((T, Cn)) + 1j * rng.standard_normal((T, Cn))).astype(NPT[dtname])
    else:
        x = rng.standard_normal((T, Cn)).astype(NPT[dtname])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def taps(K, dtname="f32", seed=9):
    h = np.random.default_rng(seed + K).standard_normal(K) / np.sqrt(K)
    h = h.astype(np.float64 if is_double(dtname) else np.float32).astype(np.float64)      # the values the device sees
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def reference(T, Cn, dtname, K, p, q, off, J, edge):
    """the restatement's result, computed once per case and never modified"""
    want = R.polyphase_fast(taps(K, dtname), data(T, Cn, dtname), p, q, off, J, edge)
    want.setflags(write=False)
    return want


def raw(x, h, p, q, off, J, edge="zero", x_ld=None, out_ld=None, stream=None, check=True):
    """the C entry on a guarded, poisoned output; the record lies in NaN (int16: 32767) surroundings.  x: numpy T x C; returns (numpy J x C, device output)."""
    T, Cn = x.shape
    dtname = {v: k for k, v in NPT.items()}[x.dtype.type]
    dbl = is_double(dtname)
    xt = torch.from_numpy(np.ascontiguousarray(x.T)).cuda()                               # C x T
    big = torch.zeros((Cn, x_ld or T), dtype=xt.dtype, device="cuda")
    big[:, :T] = xt
    xt = GD.haloed_view(big[:, :T], "nan")
    ht = torch.from_numpy(np.asarray(h, np.float64 if dbl else np.float32)).cuda()
    old = out_ld or J
    g = GD.Guard()
    out = g.empty((Cn, old), OUT[dtname], "cuda")
    d = _lib.ResampleDesc()
    d.T, d.C, d.K, d.J, d.p, d.q, d.off = T, Cn, len(h), J, p, q, off
    d.x_ld, d.out_ld = (x_ld or T), old
    d.in_type, d.edge, d.device = CODE[dtname], int(edge == "odd"), -1
    d.queue = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    _lib.check(_lib.lib().qdas_resample(C.byref(d), C.c_void_p(xt.data_ptr()), C.c_void_p(ht.data_ptr()), C.c_void_p(out.data_ptr())))
    if not check:
        return None, out
    torch.cuda.synchronize()
    g.check()                                                                             # the guard bands
    comp = torch.view_as_real(out) if out.is_complex() else out.unsqueeze(-1)
    poison = comp.view(GD._INT[comp.element_size()]) == -1
    assert not bool(poison[:, :J].any()), "every output element is written"
    assert bool(poison[:, J:].all()), "the padding behind a trace is not touched"
    return np.ascontiguousarray(out[:, :J].t().cpu().numpy()), out


def parts(a):
    a = np.ascontiguousarray(a)
    return a.view(np.float64 if a.dtype in (np.complex128, np.float64) else np.float32)


def compare(got, want, x, h, p, dtname, edge="zero", what=""):
    bd = R.bound(h, p, float(np.abs(parts(np.ascontiguousarray(x).astype(NPT[dtname] if dtname != "i16" else np.float32))).max()) if x.size else 0.0,
                 double=is_double(dtname), odd=edge == "odd")
    w = np.ascontiguousarray(want.astype(np.complex128 if np.iscomplexobj(want) else np.float64))
    gg = np.ascontiguousarray(got.astype(w.dtype))
    err = np.abs(parts(gg) - parts(w)).max() if gg.size else 0.0
    ratio = float(err / bd) if bd > 0 else float(err != 0)
    SEEN["ratio"] = max(SEEN["ratio"], ratio)
    print(f"resample ratio {what}: {ratio:.3f} (largest so far {SEEN['ratio']:.3f})")
    assert np.isfinite(parts(gg)).all()
    assert ratio <= 1.0, (what, ratio)


def one(T, Cn, dtname, K, p, q, off=None, J=None, edge="zero", **kw):
    off = (K - 1) // 2 if off is None else off
    J = R.resample_len(T, p, q) if J is None else J
    x, h = data(T, Cn, dtname), taps(K, dtname)
    want = reference(T, Cn, dtname, K, p, q, off, J, edge)
    got, _ = raw(x, h, p, q, off, J, edge, **kw)
    assert got.shape == want.shape == (J, Cn)
    assert np.iscomplexobj(got) == np.iscomplexobj(x), "the output is real for real input"
    compare(got, want, x, h, p, dtname, edge, f"T={T} C={Cn} {dtname} K={K} {p}/{q} off={off} J={J} {edge}")


# ---------------------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("p,q", [(3, 2), (2, 3)])
@pytest.mark.parametrize("J", [1, 63, 64, 65, 255, 256, 257, 513, 1025])
def test_output_counts_around_every_tile(J, p, q):
    one(max(1, J * q // p), 1, "f32", 61, p, q, J=J)


@pytest.mark.parametrize("p,q", [(3, 2), (2, 3), (16, 25)])
def test_records_around_one_q(p, q):
    for T in sorted({1, 2, max(q - 1, 1), q, q + 1}):
        one(T, 3, "f32", 2 * 3 * max(p, q) + 1, p, q)


PQ = [(1, 1), (2, 1), (1, 2), (3, 2), (2, 3), (5, 4), (4, 5), (16, 25), (25, 16), (1, 32), (32, 1), (6, 4), (7, 4096), (4096, 7)]


@pytest.mark.parametrize("p,q", PQ)
def test_rates_and_tap_counts(p, q):
    """K in {1, 2, 3, p-1, p, p+1, 61, 641}: phases with unequal tap counts and phases without taps; upfirdn's length, so that the last taps are met"""
    T = 3 * 4096 // p + 300 if q == 4096 else max(8, min(1200, 300 * q // p))
    for K in sorted({1, 2, 3, max(p - 1, 1), p, p + 1, 61, 641}):
        one(T, 1, "f32", K, p, q, off=0, J=min(R.upfirdn_len(T, K, p, q), 1100))


@pytest.mark.parametrize("p,q,K", [(3, 2, 61), (1, 1, 9), (4, 5, 3), (7, 3, 5)])
def test_offsets(p, q, K):
    T = 700
    for off in sorted({0, 1, p - 1, p, (K - 1) // 2, K - 1, K + 3 * p}):
        one(T, 1, "f32", K, p, q, off=off, J=R.resample_len(T, p, q))


@pytest.mark.parametrize("p,q", [(1, 32), (32, 1)])
def test_the_accepted_extreme_designs_in_complex128(p, q):
    h = RS.resample_taps(p, q)
    assert h.size == 641
    T = 64 * 32 * 2 + 77 if q == 32 else 70
    x = data(T, 1, "c128")
    J = R.resample_len(T, p, q)
    got, _ = raw(x, h, p, q, 320, J)
    compare(got, R.polyphase_fast(h, x, p, q, 320, J), x, h, p, "c128", what=f"default design {p}/{q} complex128")


@pytest.mark.parametrize("dtname", ["i16", "f32", "c64", "f64", "c128"])
def test_the_accepted_extremes_in_every_type(dtname):
    one(64 * 32 + 99, 1, dtname, 641, 1, 32)
    Kb = 513
    one(3 * (Kb - 1) + 1, 1, dtname, 2 * Kb - 1, 1, 1, off=Kb - 1, J=3 * (Kb - 1) + 1, edge="odd")


@pytest.mark.parametrize("Kb", [2, 9, 26, 129, 513])
def test_filtfilt_shapes_as_direct_calls(Kb):
    for T in (3 * (Kb - 1) + 1, 3 * (Kb - 1) + 300):
        one(T, 1, "f32", 2 * Kb - 1, 1, 1, off=Kb - 1, J=T, edge="odd")


@pytest.mark.parametrize("p,q,K,off", [(3, 2, 31, 15), (2, 3, 31, 0), (1, 1, 40, 0), (1, 1, 1, 39), (16, 25, 101, 50)])
def test_the_odd_edge_at_other_rates_up_to_its_reach(p, q, K, off):
    T = 40 if p == q else 300
    hi = 2 * (T - 1)                                                  # the last output may read x[2 (T - 1)]: floor((off + (J - 1) q) / p) <= 2 (T - 1)
    J = ((hi + 1) * p - 1 - off) // q + 1
    lo = -(-(off - K + 1) // p)
    assert lo >= -(T - 1) and (off + (J - 1) * q) // p <= hi < (off + J * q) // p
    one(T, 2, "c64", K, p, q, off=off, J=J, edge="odd")


# ---------------------------------------------------------------------------------------------------------------- layouts and types
@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("dtname", ["i16", "f32", "c64", "f64", "c128"])
def test_types_and_trace_counts(dtname, Cn):
    one(1101, Cn, dtname, 101, 5, 4)
    one(1101, Cn, dtname, 81, 4, 5, edge="odd", J=R.resample_len(1101, 4, 5) - 40)


@pytest.mark.parametrize("dtname", ["i16", "f32", "c64", "f64", "c128"])
def test_strided_traces_in_poisoned_padding(dtname):
    T = 1030
    one(T, 3, dtname, 61, 3, 2, x_ld=T + 37, out_ld=R.resample_len(T, 3, 2) + 11)
    one(T, 3, dtname, 51, 1, 1, off=25, J=T, edge="odd", x_ld=T + 5, out_ld=T + 3)


# ---------------------------------------------------------------------------------------------------------------- what is read, what is written
def test_two_runs_give_the_same_bits():
    x, h = data(2100, 3, "i16"), taps(101)
    a, _ = raw(x, h, 5, 4, 50, 2625)
    c, _ = raw(x, h, 5, 4, 50, 2625)
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32))


@pytest.mark.parametrize("K,p,q,off,i", [(61, 3, 2, 30, 700), (101, 5, 4, 50, 1024), (9, 1, 1, 4, 1023), (33, 2, 3, 0, 801), (7, 1, 8, 3, 802), (5, 16, 25, 2, 639), (641, 1, 32, 320, 2000)])
def test_a_nan_reaches_exactly_the_outputs_that_read_it(K, p, q, off, i):
    T = 2300
    J = R.resample_len(T, p, q)
    x = np.array(data(T, 1, "f32"))
    clean, _ = raw(x, taps(K), p, q, off, J)
    x[i, 0] = np.nan
    got, _ = raw(x, taps(K), p, q, off, J)
    hit = np.zeros(J, bool)
    hit[R.reads(i, K, p, q, off, J)] = True
    assert hit.any()
    assert np.isnan(got[hit, 0]).all()
    assert np.array_equal(got[~hit].view(np.uint32), clean[~hit].view(np.uint32))


def test_samples_no_output_reads_may_hold_nan():
    """q = 8, K = 3, off = 2: output j reads x[8j], x[8j + 1], x[8j + 2]; indices = 3 .. 7 (mod 8) are NaN.  And the tail behind the last output's window.
    With p = 8, K = 3 the outputs of phases 3 .. 7 have no taps: exact zeros beside NaN-free neighbours."""
    T, q, K = 2 * 1024 * 8 + 21, 8, 3
    J = 2000
    x = np.array(data(T, 2, "f32"))
    clean, _ = raw(x, taps(K), 1, q, 2, J)
    idx = np.arange(T)
    x[(idx % 8 >= 3) | (idx > (J - 1) * q + 2)] = np.nan
    got, _ = raw(x, taps(K), 1, q, 2, J)
    assert np.isfinite(got).all() and np.array_equal(got.view(np.uint32), clean.view(np.uint32))
    x = np.array(data(300, 1, "f32"))
    got, _ = raw(x, taps(3), 8, 1, 0, 2400)
    ph = np.arange(2400) % 8
    assert (got[ph >= 3] == 0).all() and (got[ph < 3] != 0).all()
    # upsampling by 3 with J short of the record: the samples behind the last window are never multiplied
    x = np.array(data(500, 1, "f32"))
    clean, _ = raw(x, taps(7), 3, 1, 3, 600)
    x[(600 - 1 + 3) // 3 + 1:] = np.nan
    got, _ = raw(x, taps(7), 3, 1, 3, 600)
    assert np.array_equal(got.view(np.uint32), clean.view(np.uint32))


def desc(**kw):
    d = _lib.ResampleDesc()
    d.T, d.C, d.K, d.J, d.p, d.q, d.off, d.x_ld, d.out_ld = 100, 2, 5, 150, 3, 2, 2, 100, 150
    d.in_type, d.edge, d.device = _lib.RESAMPLE_F32, _lib.RESAMPLE_ZERO, -1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_an_empty_call_launches_nothing():
    L = _lib.lib()
    for kw in (dict(J=0), dict(C=0)):
        g = GD.Guard()
        out = g.empty((2, 150), torch.float32, "cuda")
        assert L.qdas_resample(C.byref(desc(**kw)), None, None, C.c_void_p(out.data_ptr())) == 0
        assert L.qdas_resample(C.byref(desc(**kw)), None, None, None) == 0
        torch.cuda.synchronize()
        g.check()
        assert bool((out.view(torch.int32) == -1).all()), "nothing was written"


def test_refusals_return_their_codes():
    L = _lib.lib()
    x = torch.zeros(200, device="cuda")
    h = torch.zeros(5, device="cuda")
    g = GD.Guard()
    out = g.empty((2, 150), torch.float32, "cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    call = lambda d, xx=x, hh=h, oo=out: L.qdas_resample(C.byref(d) if d is not None else None, ptr(xx) if xx is not None else None,
                                                          ptr(hh) if hh is not None else None, ptr(oo) if oo is not None else None)
    assert call(None) == 1
    for kw in (dict(p=0), dict(q=0), dict(K=0), dict(x_ld=99), dict(out_ld=149), dict(in_type=5), dict(in_type=-1), dict(edge=2), dict(T=0, x_ld=0),
               dict(edge=1, p=1, q=1, off=0, K=101), dict(edge=1, p=1, q=1, off=60, K=1)):
        assert call(desc(**kw)) == 1, kw
        assert b"resample" in L.qdas_last_error()
    assert call(desc(), xx=None) == 1 and call(desc(), hh=None) == 1 and call(desc(), oo=None) == 1
    assert call(desc(K=_lib.RESAMPLE_MAX_K + 1)) == _lib.QDAS_EUNSUPPORTED
    assert call(desc(p=_lib.RESAMPLE_MAX_PQ + 1)) == _lib.QDAS_EUNSUPPORTED and call(desc(q=_lib.RESAMPLE_MAX_PQ + 1)) == _lib.QDAS_EUNSUPPORTED
    assert call(desc(K=4096, p=1, q=1, in_type=_lib.RESAMPLE_C128)) == _lib.QDAS_EUNSUPPORTED, "the LDS budget"
    torch.cuda.synchronize()
    g.check()
    assert bool((out.view(torch.int32) == -1).all()), "a refused call writes nothing"


# ---------------------------------------------------------------------------------------------------------------- stream
def test_stream_delayed_producer_on_a_side_stream():
    from tests.test_gpu_raybackproject import own_stream
    T, Cn, K, p, q = 2100, 3, 101, 5, 4
    J = R.resample_len(T, p, q)
    x, h = data(T, Cn, "f32"), taps(K)
    want = reference(T, Cn, "f32", K, p, q, 50, J, "zero")
    xt = torch.from_numpy(np.ascontiguousarray(x.T)).cuda()
    ht = torch.from_numpy(h.astype(np.float32)).cuda()
    g = GD.Guard()

    def fn(xx, hh):
        out = g.empty((Cn, J), torch.float32, "cuda")
        d = desc(T=T, C=Cn, K=K, J=J, p=p, q=q, off=50, x_ld=T, out_ld=J)
        d.queue = C.c_void_p(side.cuda_stream)
        _lib.check(_lib.lib().qdas_resample(C.byref(d), C.c_void_p(xx.data_ptr()), C.c_void_p(hh.data_ptr()), C.c_void_p(out.data_ptr())))
        return out

    with own_stream() as side:                          # (not torch.cuda.Stream(): a pool stream lives on and moves the later files' streams to other hardware queues)
        (out,), (clone,), early = ST.run_delayed(fn, [xt, ht], side, FILL_MS)
    assert early, "the entry returned while the producer was still running: it synchronises nothing"
    g.check(out, all_written=True)                          # the guard bands, and every element written
    assert ST.same_bits(out, clone)
    compare(out.t().cpu().numpy(), want, x, h, p, "f32", what="side stream")


# ---------------------------------------------------------------------------------------------------------------- the Python layer
def test_python_functions_against_scipy(monkeypatch):
    from scipy.signal import filtfilt, resample_poly, upfirdn
    T = 700
    x = data(T, 6, "c64").reshape(T, 3, 2)
    xt = torch.from_numpy(np.array(x)).cuda()
    with GD.guard_outputs(monkeypatch) as g:
        for p, q in ((3, 2), (16, 25), (6, 4)):
            got = RS.resample(xt, p, q)
            g.check(got)
            pr, qr = np.array([p, q]) // np.gcd(p, q)
            h = RS.resample_taps(p, q)
            want = resample_poly(x.astype(np.complex128), pr, qr, axis=0, window=h / pr)
            compare(got.cpu().numpy().reshape(-1, 1), want.reshape(-1, 1), x, h.astype(np.float32).astype(np.float64), pr, "c64", what=f"resample {p}/{q} vs resample_poly")
        h = taps(23)
        got = RS.upfirdn(h, xt, 3, 2)
        g.check(got)
        compare(got.cpu().numpy().reshape(-1, 1), upfirdn(h, x.astype(np.complex128), 3, 2, axis=0).reshape(-1, 1), x, h, 3, "c64", what="upfirdn vs scipy")
        b = taps(26)
        got = RS.filtfilt(b, xt)
        g.check(got)
        c = RS.filtfilt_taps(b)
        compare(got.cpu().numpy().reshape(-1, 1), filtfilt(b, [1.0], x.astype(np.complex128), axis=0, padlen=75).reshape(-1, 1), x, c.astype(np.float32).astype(np.float64), 1,
                "c64", edge="odd", what="filtfilt vs scipy")
    same = RS.resample(xt, 4, 4)
    assert same.data_ptr() != xt.data_ptr() and torch.equal(same, xt), "p = q: a copy"
    real = RS.resample(torch.from_numpy(np.array(data(300, 2, "i16"))).cuda(), 2, 3)
    assert real.dtype == torch.float32 and tuple(real.shape) == (200, 2)


@pytest.mark.parametrize("order", ["TNM", "NTM"])
def test_channeldata_methods(order, monkeypatch):
    from scipy.signal import filtfilt, resample_poly
    T, N, M, fs = 801, 3, 2, 62.5e6
    x = data(T, N * M, "f32").reshape(T, N, M)
    t0 = np.array([1.1e-6, -0.4e-6]).reshape(1, 1, M)
    perm = [("TNM").index(c) for c in order]
    chd = ChannelData(torch.from_numpy(np.ascontiguousarray(x.transpose(perm))).cuda(), t0.transpose(perm), fs, order)
    ax = order.index("T")
    with GD.guard_outputs(monkeypatch) as g:
        got = chd.resample(40e6)
        g.check(got.data)
        ff = chd.filtfilt(taps(26))
        g.check(ff.data)
    h = RS.resample_taps(16, 25)
    assert got.order == order and got.fs == fs * 16 / 25 == 40e6 and got.t0 is chd.t0 and got.data.shape[ax] == R.resample_len(T, 16, 25)
    want = resample_poly(x.astype(np.float64), 16, 25, axis=0, window=h / 16).transpose(perm)
    compare(got.data.cpu().numpy().reshape(-1, 1), want.reshape(-1, 1), x, h.astype(np.float32).astype(np.float64), 16, "f32", what=f"ChannelData.resample {order}")
    b = taps(26)
    assert ff.order == order and ff.fs == fs and ff.t0 is chd.t0 and tuple(ff.data.shape) == tuple(chd.data.shape)
    want = filtfilt(b, [1.0], x.astype(np.float64), axis=0, padlen=75).transpose(perm)
    compare(ff.data.cpu().numpy().reshape(-1, 1), want.reshape(-1, 1), x, RS.filtfilt_taps(b).astype(np.float32).astype(np.float64), 1, "f32", edge="odd",
            what=f"ChannelData.filtfilt {order}")
    for K in (26, 301):
        f1, f2 = chd.fftfilt(taps(K)), chd.filter(taps(K))
        assert torch.equal(f1.data, f2.data) and np.array_equal(np.asarray(f1.t0), np.asarray(f2.t0)) and f1.fs == fs and f1.order == order
        assert np.allclose(np.asarray(f1.t0), t0.transpose(perm) - (K - 1) / 2 / fs, rtol=0, atol=1e-18)
    up = chd.resample(0.0, p=6, q=4)
    assert up.fs == fs * 1.5 and up.data.shape[ax] == R.resample_len(T, 3, 2)


def test_a_tone_resampled_five_fourths():
    """interior outputs 100 .. 399 stay within twice the error the float64 restatement gives for the same input: the design's own ripple (1.63e-3)"""
    t = np.arange(400.0)
    x = np.cos(2 * np.pi * 0.05 * t)[:, None]
    j = np.arange(100, 400)
    tone = np.cos(2 * np.pi * 0.05 * j * 4 / 5)
    ripple = np.abs(R.resample(x, 5, 4, RS.resample_taps(5, 4))[j, 0] - tone).max()
    for dt in (torch.float32, torch.float64):
        y = RS.resample(torch.from_numpy(x).to(dt).cuda(), 5, 4).cpu().numpy()[:, 0]
        err = np.abs(y[j] - tone).max()
        print(f"resample tone {dt}: {err:.3e} against the restatement's {ripple:.3e}")
        assert y.shape == (500,) and err <= 2 * ripple


def test_python_layer_refuses_what_it_cannot_take():
    x = torch.zeros(64, 2, device="cuda")
    chd = ChannelData(x, 0.0, 20e6)
    with pytest.raises(DasError, match="IIR"):
        chd.filtfilt([1.0, 0.5], a=[1.0, -0.5])
    with pytest.raises(DasError, match="IIR"):
        chd.filtfilt(None, sos=np.ones((1, 6)))
    with pytest.raises(DasError, match=r"more than 3 \(K - 1\)"):
        chd.filtfilt(np.ones(23))
    with pytest.raises(DasError, match=r"more than 3 \(K - 1\)"):
        RS.filtfilt(np.ones(23), x)
    for call in (lambda: RS.resample(x.cpu(), 3, 2), lambda: RS.filtfilt([0.5, 0.5], x.cpu()), lambda: RS.upfirdn([1.0], x.cpu(), 2, 1)):
        with pytest.raises(DasError, match="device tensor"):
            call()
    with pytest.raises(DasError):
        RS.resample(x, 3, 0)
    with pytest.raises(DasError):
        RS.resample(x, 3, 2, h=np.ones(4))
    with pytest.raises(DasError):
        RS.resample(x.half(), 3, 2)
    with pytest.raises(DasError, match="explicit"):
        chd.resample(20e6 * np.pi / 3)
    with pytest.raises(_lib.QdasError) as e:
        RS.upfirdn(np.ones(_lib.RESAMPLE_MAX_K + 1), x, 2, 1)
    assert e.value.code == _lib.QDAS_EUNSUPPORTED


def test_greens_to_resample_to_das_peaks_where_the_unresampled_route_does():
    """the geometry of the demod test: one scatterer on a pixel of a grid with a pitch of about a resolution cell; real float32 RF -> resample to 5/4 of the
    rate -> hilbert -> DAS peaks on the pixel hilbert -> DAS peaks on"""
    fc, c0 = 5e6, 1500.0
    fs = 8 * fc
    xdc = Transducer.linear(16, 0.3e-3, fc)
    xs, zs = np.linspace(-2e-3, 2e-3, 11), np.linspace(8e-3, 12e-3, 17)
    us = UltrasoundSystem(xdc, Sequence("FSA", c0=c0), Scan.cartesian(xs, zs), fs=fs)
    t = np.arange(-2.0 / fc, 2.0 / fc, 1 / (4 * fs))
    wv = np.exp(-(t * fc * 1.2) ** 2) * np.exp(2j * np.pi * fc * t)
    chd = us.greens(np.array([[0.4e-3], [0.0], [10.25e-3]]), [1.0], wv, t[0], 4 * fs, R0=c0 / fc)
    d = chd.data if hasattr(chd.data, "is_cuda") else torch.from_numpy(np.asarray(chd.data))
    rf = torch.real(d).float().contiguous().cuda() if d.is_complex() else d.float().cuda()
    rf = ChannelData(rf / rf.abs().max(), chd.t0, chd.fs, chd.order)
    b_ref = us.DAS(rf.hilbert())
    peak = int(b_ref.abs().flatten().argmax())
    assert peak == 9 * 11 + 6, "the scatterer's pixel (z index 9, x index 6)"
    rs = rf.resample(rf.fs * 5 / 4)
    assert rs.fs == rf.fs * 5 / 4 and rs.T == R.resample_len(rf.T, 5, 4)
    b_rs = us.DAS(rs.hilbert())
    rel = float((b_rs - b_ref).abs().max() / b_ref.abs().max())
    print(f"resample route: max|b_rs - b_ref| / max|b_ref| = {rel:.2e}; peaks {int(b_rs.abs().flatten().argmax())} / {peak}")
    assert int(b_rs.abs().flatten().argmax()) == peak
