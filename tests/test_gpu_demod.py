"""qdas_demod and its Python layer (qups_amd/demod.py, ChannelData.demod) on the device, against the float64 restatement tests/demod_ref.py -- by definition
``downmix(fc).filter(b).downsample(R)``.

TOLERANCE per element, derived and not tuned: ``|err| <= ((K + 8) eps + 8 pi eps64 max|fc t|) sum|b| max|x|`` with eps = 2^-24 (2^-53 for double data), plus
``2^-11 |ref|`` for half output (tests/demod_ref.py ``bound``).  K products of one rounding each and K - 1 sums give the first term; the three float64 phase
reductions the second.  The data and the taps are random normal, so a dropped tap or a wrong phase is an error of the order of ``|b_k| max|x|`` -- hundreds of
bounds.  The largest measured ratio err / bound over every case of this file on one MI355X (every case prints its own as ``demod ratio``): 0.167 with
complex64 / complex128 output (K = 1: the two phase roundings beside a single product), 0.887 with half output, whose bound is the half rounding itself;
``ChannelData.demod`` against the composition of the same object, held to the same bound: see test_channeldata_demod_is_the_composition.

JT = 256 outputs per workgroup (``QDAS_DEMOD_TILE``); at most ``QDAS_DEMOD_MAX_K`` = 1024 taps, ``QDAS_DEMOD_MAX_R`` = 4096.

The entry takes its stream in the descriptor's ``queue`` field (the census of ``void *stream`` parameters, tests/test_streams_host.py, is a pinned list): the
stream case is in this file."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from qups_amd import ChannelData, DasError, Scan, Sequence, Transducer, UltrasoundSystem, _lib
from qups_amd.demod import demod as py_demod
from tests import demod_ref as R
from tests import guards as GD
from tests import streams as ST

pytestmark = pytest.mark.gpu

JT, MAXK, MAXR = _lib.DEMOD_TILE, _lib.DEMOD_MAX_K, _lib.DEMOD_MAX_R
FC, FS, T0 = 5.1e6, 20e6, 3.3e-6
NPT = {"i16": np.int16, "f32": np.float32, "c64": np.complex64, "f64": np.float64, "c128": np.complex128}
CODE = {"i16": _lib.DEMOD_I16, "f32": _lib.DEMOD_F32, "c64": _lib.DEMOD_C64, "f64": _lib.DEMOD_F64, "c128": _lib.DEMOD_C128}
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
    b = np.random.default_rng(seed + K).standard_normal(K) / np.sqrt(K)
    b = b.astype(np.float64 if is_double(dtname) else np.float32).astype(np.float64)      # the values the device sees
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def reference(T, Cn, dtname, K, ratio, t0key):
    """the restatement's result, computed once per case and never modified"""
    t0 = np.asarray(t0key, np.float64)
    want = R.demod(data(T, Cn, dtname), FC, FS, t0.reshape(1, -1) if t0.size > 1 else float(t0.reshape(-1)[0]), taps(K, dtname), ratio)
    want.setflags(write=False)
    return want


def raw(x, b, ratio, cyc0, gdiv=1, fc_over_fs=FC / FS, out_half=False, x_ld=None, out_ld=None, stream=None, xt=None, check=True):
    """the C entry on a guarded, poisoned output.  x: numpy T x C; returns (numpy J x C complex, the device output C x out_ld).  With x_ld / out_ld the traces
    lie in poisoned padding."""
    T, Cn = x.shape
    dtname = {v: k for k, v in NPT.items()}[x.dtype.type]
    dbl = is_double(dtname)
    J = R_len(T, ratio)
    if xt is None:
        xt = torch.from_numpy(np.ascontiguousarray(x.T)).cuda()                           # C x T
        if x_ld is not None:
            big = torch.zeros((Cn, x_ld), dtype=xt.dtype, device="cuda")
            big[:, :T] = xt
            xt = GD.haloed_view(big[:, :T], "nan")
    bt = torch.from_numpy(np.asarray(b, np.float64 if dbl else np.float32)).cuda()
    ct = torch.from_numpy(np.atleast_1d(np.asarray(cyc0, np.float64))).cuda()
    old = out_ld or J
    g = GD.Guard()
    odt = torch.float16 if out_half else (torch.complex128 if dbl else torch.complex64)
    out = g.empty((Cn, old, 2) if out_half else (Cn, old), odt, "cuda")
    d = _lib.DemodDesc()
    d.T, d.C, d.K, d.R = T, Cn, len(b), ratio
    d.x_ld, d.out_ld = (xt.stride(0) if Cn > 1 else max(T, x_ld or T)), old
    d.in_type, d.out_half, d.device = CODE[dtname], int(out_half), -1
    d.fc_over_fs, d.step = fc_over_fs, fc_over_fs * ratio
    d.cyc0, d.gdiv, d.G = C.c_void_p(ct.data_ptr()), gdiv, ct.numel()
    d.queue = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    _lib.check(_lib.lib().qdas_demod(C.byref(d), C.c_void_p(xt.data_ptr()), C.c_void_p(bt.data_ptr()), C.c_void_p(out.data_ptr())))
    if not check:
        return None, out
    torch.cuda.synchronize()
    g.check()                                                                             # the guard bands
    o = torch.view_as_complex(out.float()) if out_half else out
    comp = out if out_half else torch.view_as_real(out)                                   # C x out_ld x 2 real scalars
    poison = comp.view(GD._INT[comp.element_size()]) == -1
    assert not bool(poison[:, :J].any()), "every output element is written"
    assert bool(poison[:, J:].all()), "the padding behind a trace is not touched"
    return np.ascontiguousarray(o[:, :J].t().cpu().numpy()), out


def R_len(T, ratio):
    return -(-T // ratio)


def cyc_of(t0):
    c = FC * np.asarray(t0, np.float64)
    return c - np.floor(c)


def compare(got, want, x, b, dtname, t0max, out_half=False, what=""):
    T = x.shape[0]
    got = np.ascontiguousarray(got)
    bd = R.bound(len(b), b, np.abs(x).max() if x.size else 0.0, FC * (abs(t0max) + T / FS), double=is_double(dtname))
    err = np.abs(got - want)
    tol = bd + (2.0 ** -11 * np.abs(want) if out_half else 0.0)
    ratio = float((err / tol).max()) if err.size else 0.0
    SEEN["ratio"] = max(SEEN["ratio"], ratio)
    print(f"demod ratio {what}: {ratio:.3f} (largest so far {SEEN['ratio']:.3f})")
    assert np.isfinite(got.view(np.float64 if got.dtype == np.complex128 else np.float32)).all()
    assert ratio <= 1.0, (what, ratio)


def one(T, Cn, dtname, K, ratio, out_half=False, t0=T0, gdiv=1, **kw):
    x, b = data(T, Cn, dtname), taps(K, dtname)
    t0key = tuple(np.atleast_1d(t0).tolist())
    if len(t0key) > 1:                                                                    # trace c starts at t0[(c // gdiv) % G]
        per_trace = tuple(t0key[(c // gdiv) % len(t0key)] for c in range(Cn))
        want = reference(T, Cn, dtname, K, ratio, per_trace)
    else:
        want = reference(T, Cn, dtname, K, ratio, t0key)
    got, _ = raw(x, b, ratio, cyc_of(t0), gdiv=gdiv, out_half=out_half, **kw)
    assert got.shape == want.shape == (R_len(T, ratio), Cn)
    compare(got, want, x, b, dtname, np.abs(t0key).max(), out_half, f"T={T} C={Cn} {dtname} K={K} R={ratio} half={int(out_half)}")


# ---------------------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("J", [1, JT - 1, JT, JT + 1, 2 * JT + 1])
def test_output_counts_around_the_tile(J):
    one(4 * J - 2, 1, "f32", 25, 4)


@pytest.mark.parametrize("T", [1, 3, 4, 5])
def test_records_around_one_ratio(T):
    one(T, 3, "f32", 25, 4)


@pytest.mark.parametrize("K", [1, 2, 25, 26, 129])
def test_tap_counts(K):
    one(1501, 3, "f32", K, 4)


def test_taps_span_more_than_a_tiles_own_inputs():
    assert 300 > JT * 1
    one(601, 1, "f32", 300, 1)
    one(2 * JT * 2 + 3, 1, "f32", JT * 2 + 7, 2)


def test_more_taps_than_samples():
    one(50, 3, "f32", 129, 4)


@pytest.mark.parametrize("ratio", [1, 4, 64])
def test_the_largest_tap_count(ratio):
    one(JT * ratio + 2100, 1, "f32", MAXK, ratio)


@pytest.mark.parametrize("dtname", ["c64", "f64", "c128"])
def test_the_largest_tap_count_in_the_wide_types(dtname):
    one(1400, 1, dtname, MAXK, 1)


@pytest.mark.parametrize("ratio", [1, 2, 3, 4, 8, 16, MAXR])
def test_ratios(ratio):
    one((JT + 1) * ratio + 3 if ratio < MAXR else 3 * ratio + 5, 3, "f32", 33, ratio)


def test_the_largest_ratio_with_the_largest_tap_count():
    one(3 * MAXR + 5, 1, "f32", MAXK, MAXR)


@pytest.mark.parametrize("ratio", [9, 13])
def test_ratios_staged_in_two_phase_groups(ratio):
    one((JT + 1) * ratio + 3, 1, "f32", 4 * ratio + 1, ratio)


# ---------------------------------------------------------------------------------------------------------------- layouts and types
@pytest.mark.parametrize("Cn", [1, 3])
def test_trace_counts(Cn):
    one(1201, Cn, "i16", 25, 4)


def test_one_start_time_per_transmit():
    N, M = 3, 2
    one(1201, N * M, "f32", 25, 4, t0=(T0, -1.7e-6), gdiv=N)


@pytest.mark.parametrize("dtname", ["i16", "f32", "c64", "f64"])
def test_strided_traces_in_poisoned_padding(dtname):
    T, ratio = 1030, 4
    one(T, 3, dtname, 26, ratio, x_ld=T + 37, out_ld=R_len(T, ratio) + 11)


@pytest.mark.parametrize("dtname,out_half", [("i16", False), ("i16", True), ("f32", False), ("f32", True), ("c64", False), ("c64", True), ("f64", False),
                                             ("c128", False)])
def test_types(dtname, out_half):
    one(1101, 3, dtname, 25, 4, out_half=out_half)
    one(1101, 1, dtname, 129, 3, out_half=out_half)


# ---------------------------------------------------------------------------------------------------------------- what is read, what is written
def test_samples_no_output_reads_are_not_touched():
    """R = 8, K = 3: outputs read x[8j], x[8j - 1], x[8j - 2]; indices = 1 .. 5 (mod 8) are NaN and nothing multiplies them by zero"""
    T, ratio, K = 2 * JT * 8 + 21, 8, 3
    x = np.array(data(T, 2, "f32"))
    clean, _ = raw(x, taps(K), ratio, cyc_of(T0))
    idx = np.arange(T)
    x[(idx % 8 >= 1) & (idx % 8 <= 5)] = np.nan
    got, _ = raw(x, taps(K), ratio, cyc_of(T0))
    assert np.isfinite(got.view(np.float32)).all()
    assert np.array_equal(got.view(np.uint32), clean.view(np.uint32))


@pytest.mark.parametrize("K,ratio,i", [(25, 4, 1030), (26, 4, 1021), (129, 3, 700), (7, 8, 802), (33, 1, 255), (5, 16, 4096 + 16 * 3)])
def test_a_nan_reaches_exactly_the_outputs_that_read_it(K, ratio, i):
    T = 2 * JT * ratio + 77
    x = np.array(data(T, 1, "f32"))
    clean, _ = raw(x, taps(K), ratio, cyc_of(T0))
    x[i, 0] = np.nan
    got, _ = raw(x, taps(K), ratio, cyc_of(T0))
    hit = np.zeros(got.shape[0], bool)
    hit[R.nan_reach(i, K, ratio, got.shape[0])] = True
    assert hit.any()
    assert np.isnan(got[hit, 0].real).all() and np.isnan(got[hit, 0].imag).all()
    assert np.array_equal(got[~hit].view(np.uint32), clean[~hit].view(np.uint32))


def test_two_runs_give_the_same_bits():
    x, b = data(2 * JT * 4 + 9, 3, "i16"), taps(129)
    a, _ = raw(x, b, 4, cyc_of(T0))
    c, _ = raw(x, b, 4, cyc_of(T0))
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32))


def desc(**kw):
    d = _lib.DemodDesc()
    d.T, d.C, d.K, d.R, d.x_ld, d.out_ld = 100, 2, 5, 4, 100, 25
    d.in_type, d.out_half, d.device = _lib.DEMOD_F32, 0, -1
    d.fc_over_fs, d.step, d.gdiv, d.G = 0.25, 1.0, 1, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_an_empty_call_launches_nothing():
    L = _lib.lib()
    for kw in (dict(T=0, out_ld=0), dict(C=0)):
        g = GD.Guard()
        out = g.empty((2, 25), torch.complex64, "cuda")
        assert L.qdas_demod(C.byref(desc(**kw)), None, None, C.c_void_p(out.data_ptr())) == 0
        assert L.qdas_demod(C.byref(desc(**kw)), None, None, None) == 0
        torch.cuda.synchronize()
        g.check()
        assert bool((torch.view_as_real(out).view(torch.int32) == -1).all()), "nothing was written"


def test_refusals_return_their_codes():
    L = _lib.lib()
    x = torch.zeros(200, device="cuda")
    b = torch.zeros(5, device="cuda")
    cy = torch.zeros(1, dtype=torch.float64, device="cuda")
    g = GD.Guard()
    out = g.empty((2, 25), torch.complex64, "cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    call = lambda d, xx=x, bb=b, oo=out: L.qdas_demod(C.byref(d) if d is not None else None, ptr(xx) if xx is not None else None,
                                                       ptr(bb) if bb is not None else None, ptr(oo) if oo is not None else None)
    ok = dict(cyc0=ptr(cy))
    assert call(None) == 1
    for kw in (dict(R=0), dict(K=0), dict(x_ld=99), dict(out_ld=24), dict(in_type=5), dict(in_type=-1), dict(out_half=2), dict(G=0), dict(gdiv=0),
               dict(fc_over_fs=float("nan")), dict(step=float("inf")), dict(in_type=_lib.DEMOD_F64, out_half=1), dict(in_type=_lib.DEMOD_C128, out_half=1)):
        assert call(desc(**ok, **kw)) == 1, kw
        assert b"demod" in L.qdas_last_error()
    assert call(desc()) == 1, "null cyc0"
    assert call(desc(**ok), xx=None) == 1 and call(desc(**ok), bb=None) == 1 and call(desc(**ok), oo=None) == 1
    assert call(desc(**ok, K=MAXK + 1)) == _lib.QDAS_EUNSUPPORTED
    assert call(desc(**ok, R=MAXR + 1, out_ld=1)) == _lib.QDAS_EUNSUPPORTED
    torch.cuda.synchronize()
    g.check()
    assert bool((torch.view_as_real(out).view(torch.int32) == -1).all()), "a refused call writes nothing"


# ---------------------------------------------------------------------------------------------------------------- stream
def test_stream_delayed_producer_on_a_side_stream():
    from tests.test_gpu_raybackproject import own_stream
    T, Cn, K, ratio = 2 * JT * 4 + 9, 3, 25, 4
    x, b = data(T, Cn, "f32"), taps(K)
    want = reference(T, Cn, "f32", K, ratio, (T0,))
    xt = torch.from_numpy(np.ascontiguousarray(x.T)).cuda()
    bt = torch.from_numpy(b.astype(np.float32)).cuda()
    ct = torch.from_numpy(np.atleast_1d(cyc_of(T0))).cuda()

    g = GD.Guard()

    def fn(xx, bb, cc):
        out = g.empty((Cn, R_len(T, ratio)), torch.complex64, "cuda")
        d = desc(T=T, C=Cn, K=K, R=ratio, x_ld=T, out_ld=R_len(T, ratio), fc_over_fs=FC / FS, step=FC / FS * ratio, cyc0=C.c_void_p(cc.data_ptr()))
        d.queue = C.c_void_p(side.cuda_stream)
        _lib.check(_lib.lib().qdas_demod(C.byref(d), C.c_void_p(xx.data_ptr()), C.c_void_p(bb.data_ptr()), C.c_void_p(out.data_ptr())))
        return out

    with own_stream() as side:                          # (not torch.cuda.Stream(): a pool stream lives on and moves the later files' streams to other hardware queues)
        (out,), (clone,), early = ST.run_delayed(fn, [xt, bt, ct], side, FILL_MS)
    assert early, "the entry returned while the producer was still running: it synchronises nothing"
    g.check(out, all_written=True)                          # the guard bands, and every element written
    assert ST.same_bits(out, clone)
    compare(out.t().cpu().numpy(), want, x, b, "f32", T0, what="side stream")


# ---------------------------------------------------------------------------------------------------------------- the Python layer
@pytest.mark.parametrize("order", ["TNM", "NTM"])
def test_channeldata_demod_is_the_composition(order, monkeypatch):
    T, N, M, K, ratio = 1101, 3, 2, 25, 4
    x = data(T, N * M, "f32").reshape(T, N, M)
    t0 = np.array([T0, -1.7e-6]).reshape(1, 1, M)
    b = taps(K)
    perm = [("TNM").index(c) for c in order]
    chd = ChannelData(torch.from_numpy(np.ascontiguousarray(x.transpose(perm))).cuda(), t0.transpose(perm), FS, order)
    with GD.guard_outputs(monkeypatch) as g:
        got = chd.demod(FC, ratio, b)
        g.check(got.data)
    comp = chd.downmix(FC).filter(b).downsample(ratio)
    assert got.order == order and got.fs == FS / ratio == comp.fs
    assert np.array_equal(np.asarray(got.t0), np.asarray(comp.t0)) and np.asarray(got.t0).shape == t0.transpose(perm).shape
    assert tuple(got.data.shape) == tuple(comp.data.shape)
    bd = R.bound(K, b, np.abs(x).max(), FC * (np.abs(t0).max() + T / FS))
    err = (got.data - comp.data).abs().max().item()
    SEEN["ratio"] = max(SEEN["ratio"], err / bd)
    print(f"demod ratio ChannelData.demod vs the composition ({order}): {err / bd:.3f} (largest so far {SEEN['ratio']:.3f})")
    assert err <= bd, "the composition of the same object, within the bound of the float64 restatement"
    want = R.demod(x, FC, FS, t0, b, ratio).transpose(perm)
    compare(got.data.cpu().numpy().reshape(-1, 1), want.reshape(-1, 1), x, b, "f32", np.abs(t0).max(), what=f"ChannelData.demod {order}")


def test_python_layer_refuses_what_it_cannot_take():
    x = torch.zeros(16, 2, device="cuda")
    with pytest.raises(DasError):
        py_demod(x.cpu(), FC, FS, 0.0, [1.0], 2)
    with pytest.raises(DasError):
        py_demod(x, FC, FS, 0.0, [1.0], 0)
    with pytest.raises(DasError):
        py_demod(x.double(), FC, FS, 0.0, [1.0], 2, out_half=True)
    with pytest.raises(_lib.QdasError) as e:
        py_demod(x, FC, FS, 0.0, np.ones(MAXK + 1), 2)
    assert e.value.code == _lib.QDAS_EUNSUPPORTED


def test_greens_to_demod_to_das_peaks_where_hilbert_to_das_does():
    """one scatterer on a pixel of a grid with a pitch of about a resolution cell (0.25 mm in depth, 0.4 mm across): real float32 RF -> demod(fc, 4, low-pass)
    -> DAS(fmod = fc) peaks on the pixel hilbert -> DAS peaks on, and so does the halfT route, whose image agrees with the single-precision one to the half
    rounding of the data (2^-11) plus the 3e-3 the suite allows the halfT DAS kernel (tests/test_gpu_golden.py)"""
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
    rf = ChannelData(rf / rf.abs().max(), chd.t0, chd.fs, chd.order)                 # unit peak: the half route keeps its eleven bits
    b_ref = us.DAS(rf.hilbert())
    peak = int(b_ref.abs().flatten().argmax())
    assert peak == 9 * 11 + 6, "the scatterer's pixel (z index 9, x index 6)"
    lp = rf.getLowpassFilter(0.6 * fc)
    b_dm = us.DAS(rf.demod(fc, 4, lp), fmod=fc)
    assert int(b_dm.abs().flatten().argmax()) == peak
    b_half = us.DAS(rf.demod(fc, 4, lp, out_half=True), fmod=fc, prec="halfT")
    h = torch.view_as_complex(torch.view_as_real(b_half).float().contiguous())
    rel = float((h - b_dm).abs().max() / b_dm.abs().max())
    print(f"demod halfT route: max|b_half - b_single| / max|b_single| = {rel:.2e}; peaks {int(h.abs().flatten().argmax())} / {peak}")
    assert rel <= 2.0 ** -11 + 3e-3
    assert int(h.abs().flatten().argmax()) == peak
