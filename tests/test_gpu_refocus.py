"""``qdas_refocus`` (csrc/refocus.hip), ``qups_amd.refocus.compose`` and ``UltrasoundSystem.refocus`` on the device against the float64 restatement
(tests/refocus_ref.py) on identical complex64 data.  Metric: ``max|y - ref| / max|ref|``.

The kernels' contract is "apply Hi": most cases use a seeded random decoder (standard normal, divided by sqrt(V), rounded to complex64 for both sides), so
that conditioning never enters.  Shapes are chosen to break staging, not to resemble a workload: radices 2 / 3 / 5 / 7 / 11, V = 1 and M = 1, N across
a 32-wide tile, V and M one 32-wide tile plus a few, several frames, the 512-thread stage path (T = 8192), a length the kernels do not take (34 = 2 x 17:
routed to ``compose``, asserted through the library's return code).

Bounds.  Largest error measured on an MI355X over every fused case of this file: 4.7e-7 (the pinv decoder of the focused sequence through
``UltrasoundSystem.refocus``; 4.1e-7 for M = 1, 3.7e-7 for the 8192-point case, 1.9e-7 to 3.3e-7 elsewhere); over every ``compose`` case: 2.4e-7.  So the
bounds are 4.7e-6 and 2.4e-6.  Each bound is ten times the measured value and never above the project's fp32 bound of 1e-4: it exists to catch indexing, shift, padding
and conjugation errors, which are O(1).

This file also holds the entry's STREAM CASES (``STREAM_CASES``): ``qdas_refocus`` takes its stream in the descriptor's ``queue`` field, because the census
of ``void *stream`` parameters (tests/test_streams_host.py) is a pinned list; a change that may edit tests/test_gpu_streams.py moves them there."""
import functools

import numpy as np
import pytest
import torch

from qups_amd import ChannelData, DasError, Scan, Sequence, Transducer, UltrasoundSystem, _lib
from qups_amd import refocus as RF
from tests import guards as GD
from tests import refocus_ref as R
from tests import streams as ST

pytestmark = pytest.mark.gpu

FS, T0 = 20e6, 1.3e-6
MEASURED_FUSED, MEASURED_COMPOSE = 4.7e-7, 2.4e-7
BOUND_FUSED, BOUND_COMPOSE = min(10 * MEASURED_FUSED, 1e-4), min(10 * MEASURED_COMPOSE, 1e-4)
FILL_MS = 16                                  # tests/test_gpu_streams.py's: ten times the largest host time of a warm wrapper call
STREAM_CASES = ("test_stream_delayed_producer_on_a_side_stream", "test_stream_two_runs_are_bit_identical",
                "test_stream_cached_t0_hit_from_a_second_stream_then_evicted_from_the_first", "test_stream_decoder_dropped_while_a_second_stream_still_reads_it")

#         T   N   V   M  frames
SHAPES = [
    (64, 5, 6, 8, 1),             # baseline
    (48, 3, 8, 8, 3),             # radix 3, frames
    (60, 33, 1, 4, 1),            # V = 1; N crosses a 32-wide tile
    (77, 2, 35, 33, 1),           # radices 7 11; V and M one tile plus a few
    (80, 4, 8, 1, 2),             # M = 1
    (770, 2, 2, 2, 1),            # radices 11 7 5 2: the 512-thread variant with two thread groups of 256 threads
    (1287, 2, 2, 2, 1),           # radices 13 11 9
]
BIG = (8192, 2, 3, 4, 1)          # the 512-thread stage path
ODD = (34, 3, 4, 4, 1)            # 17 is no radix: compose
SMALL = SHAPES[0]
IDS = lambda s: "x".join(str(v) for v in s)


@functools.lru_cache(maxsize=None)
def _data(T, N, V, M, frames, seed=0):
    """``(x, Hi)``: complex64 data ``T x N x V x frames`` and a random decoder ``M x V x T`` whose values are exactly representable in complex64"""
    rng = np.random.default_rng(seed + 1000 * T + 10 * N + V)
    x = (rng.standard_normal((T, N, V, frames)) + 1j * rng.standard_normal((T, N, V, frames))).astype(np.complex64)
    Hi = ((rng.standard_normal((M, V, T)) + 1j * rng.standard_normal((M, V, T))) / np.sqrt(V)).astype(np.complex64).astype(np.complex128)
    return x, Hi


def _t0(V, kind):
    """a scalar, or one value per pulse with non-integer t0 fs and the smallest last"""
    return T0 if kind == "scalar" else T0 + (np.arange(V)[::-1] * 0.37 + 0.21) / FS


@functools.lru_cache(maxsize=None)
def _ref(shape, kind="scalar"):
    x, Hi = _data(*shape)
    t0 = _t0(shape[2], kind)
    return R.apply(x, t0, FS, Hi), t0


def _err(y, ref, what):
    y = y.cpu().numpy()
    assert y.shape == ref.shape and y.dtype == np.complex64, (y.shape, ref.shape, y.dtype)
    e = float(np.abs(y - ref).max() / np.abs(ref).max())
    print(f"refocus {what}: rel_err={e:.3e}")
    return e


def _run(fn, shape, kind="scalar"):
    x, Hi = _data(*shape)
    (ref, t0ref), t0 = _ref(shape, kind)
    y = fn(torch.from_numpy(x).cuda(), t0, FS, RF.Decoder(Hi))
    torch.cuda.synchronize()
    assert t0ref == float(np.min(t0))
    return _err(y, ref, f"{fn.__name__} {shape} t0={kind}")


# ---------------------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fused_shapes(shape):
    assert RF.takes(shape[0])
    assert _run(RF.fused, shape) <= BOUND_FUSED


def test_fused_8192_points():
    assert RF.takes(BIG[0])
    assert _run(RF.fused, BIG) <= BOUND_FUSED


@pytest.mark.parametrize("kind", ["per-pulse", "scalar"])
def test_fused_t0(kind):
    assert _run(RF.fused, SHAPES[1], kind) <= BOUND_FUSED


def test_refocus_returns_t0_and_the_decoder_and_takes_float32():
    x, Hi = _data(*SMALL)
    (ref, _), t0 = _ref(SMALL, "per-pulse")
    y, t0o, Hi_out = RF.refocus(torch.from_numpy(x).cuda(), t0, FS, decoder=RF.Decoder(Hi))
    assert t0o == t0.min() and Hi_out.shape == Hi.shape and np.array_equal(Hi_out, Hi)
    assert _err(y, ref, "refocus per-pulse") <= BOUND_FUSED
    xr = torch.from_numpy(np.ascontiguousarray(x.real)).cuda()
    yr, _, _ = RF.refocus(xr, T0, FS, decoder=RF.Decoder(Hi))
    assert _err(yr, R.apply(x.real, T0, FS, Hi)[0], "refocus float32") <= BOUND_FUSED
    with pytest.raises(DasError, match="half precision"):
        RF.refocus(xr.half(), T0, FS, decoder=RF.Decoder(Hi))


def test_results_are_bit_reproducible():
    x, Hi = _data(*SHAPES[3])
    xd, dec = torch.from_numpy(x).cuda(), RF.Decoder(Hi)
    assert torch.equal(RF.fused(xd, T0, FS, dec), RF.fused(xd, T0, FS, dec))


def test_fused_noncontiguous_view_and_extra_frame_dimensions():
    T, N, V, M, _ = SMALL
    x, Hi = _data(T, N, V, M, 6)
    ref = R.apply(x, T0, FS, Hi)[0].reshape(T, N, M, 2, 3)
    big = torch.zeros((2 * T, N + 3, V, 2, 3), dtype=torch.complex64, device="cuda")
    big[::2, 1:N + 1] = torch.from_numpy(x.reshape(T, N, V, 2, 3)).cuda()
    view = big[::2, 1:N + 1]
    assert not view.is_contiguous()
    assert _err(RF.fused(view, T0, FS, RF.Decoder(Hi)), ref, "view") <= BOUND_FUSED


def test_length_with_radix_17_is_routed_to_compose():
    x, Hi = _data(*ODD)
    xd, dec = torch.from_numpy(x).cuda(), RF.Decoder(Hi)
    with pytest.raises(_lib.QdasError) as e:
        RF.fused(xd, T0, FS, dec)
    assert e.value.code == _lib.QDAS_ENOTLDS and not RF.takes(ODD[0])
    (ref, _), _ = _ref(ODD)
    y, t0o, _ = RF.refocus(xd, T0, FS, decoder=dec)
    assert t0o == T0 and _err(y, ref, "refocus 34 -> compose") <= BOUND_COMPOSE
    assert _err(RF.compose(xd, T0, FS, dec), ref, "compose 34") <= BOUND_COMPOSE


@pytest.mark.parametrize("shape", SHAPES[:4], ids=IDS)
def test_compose_shapes(shape):
    assert _run(RF.compose, shape) <= BOUND_COMPOSE
    assert _run(RF.compose, shape, "per-pulse") <= BOUND_COMPOSE


def test_compose_complex128_is_the_route_of_double_data():
    x, Hi = _data(*SMALL)
    (ref, _), t0 = _ref(SMALL, "per-pulse")
    y, _, _ = RF.refocus(torch.from_numpy(x.astype(np.complex128)).cuda(), t0, FS, decoder=RF.Decoder(Hi))
    assert y.dtype == torch.complex128
    assert float(np.abs(y.cpu().numpy() - ref).max() / np.abs(ref).max()) <= 1e-12


# ---------------------------------------------------------------------------------------------------------------- real decoders
class _ApodSequence(Sequence):
    """a Sequence whose transmit apodization is a given ``M x V`` table (``Sequence.apodization`` only knows ones and the identity)"""
    apd = None

    def apodization(self, tx):
        return self.apd


def _fc_system(V=6, M=8, N=5):
    tau, pos, foci = R.fc_sequence(M, V)
    xdc = Transducer.linear(M, 0.3e-3)
    assert np.allclose(xdc.positions(), pos)
    seq = _ApodSequence("FC", foci, 1540.0)
    seq.apd = np.random.default_rng(7).uniform(0.5, 1.5, (M, V))
    us = UltrasoundSystem(xdc, seq, Scan.cartesian(np.linspace(-1e-3, 1e-3, 3), np.linspace(5e-3, 6e-3, 4)), fs=FS)
    assert np.allclose(seq.delays(xdc), tau, rtol=1e-13, atol=0)
    return us, seq, tau


@pytest.mark.parametrize("method", RF.METHODS)
def test_methods_through_ultrasoundsystem_refocus(method):
    """the focused sequence of tests/test_refocus_host.py (8 elements, 6 foci, T = 48, the seeded apodization: every method is well conditioned there),
    per-pulse t0, two frames; the decoder is built once for the two calls"""
    us, seq, tau = _fc_system()
    T, N, V, M = 48, 5, 6, 8
    x, _ = _data(T, N, V, M, 2)
    t0 = _t0(V, "per-pulse").reshape(1, 1, V)
    ref, t0ref, Hi_ref = R.refocus(x, t0, FS, tau, seq.apd, method)
    chd = ChannelData(torch.from_numpy(x), t0, FS)
    out, Hi = us.refocus(chd, method=method)
    torch.cuda.synchronize()
    assert isinstance(out, ChannelData) and out.t0 == t0ref and out.fs == FS and out.order == "TNM"
    assert Hi.shape == (M, V, T) and np.abs(Hi - Hi_ref).max() / np.abs(Hi_ref).max() <= 1e-9
    assert _err(out.data, ref, f"us.refocus {method}") <= BOUND_FUSED
    kept = us._refocus_decoder[1]
    out2, _ = us.refocus(ChannelData(torch.from_numpy(x).cuda(), t0, FS), seq, method=method)
    assert us._refocus_decoder[1] is kept and torch.equal(out2.data, out.data)
    us.refocus(chd, method=method, gamma=3.0)
    assert (us._refocus_decoder[1] is kept) == (method != "tikhonov")           # gamma is read by tikhonov only
    # a permuted ChannelData is put in order first
    outp, _ = us.refocus(ChannelData(torch.from_numpy(x).cuda().permute(1, 0, 2, 3), np.transpose(t0, (1, 0, 2)), FS, "NTM"), method=method, gamma=None)
    assert torch.equal(outp.data, out.data)


@pytest.mark.parametrize("method,gamma", [("adjoint", None), ("tikhonov", 0.0)])
def test_hadamard_identity_on_the_device(method, gamma):
    T, N, M = 32, 3, 8
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((T, N, M)) + 1j * rng.standard_normal((T, N, M))).astype(np.complex64)
    a, d = R.hadamard(M), rng.integers(0, T // 2, M)
    tau = np.broadcast_to(d[None, :] / FS, (M, M))
    xe = R.hadamard_encode(x.astype(np.complex128), a, d).astype(np.complex64)          # (sums of 8 complex64 values with +-1: exact up to rounding)
    y, t0o, _ = RF.refocus(torch.from_numpy(xe).cuda(), T0, FS, tau, a, method, gamma)
    assert t0o == T0 and _err(y, x.astype(np.complex128), f"hadamard {method}") <= BOUND_FUSED


# ---------------------------------------------------------------------------------------------------------------- memory guards
def _serial(shape, kind="per-pulse"):
    x, Hi = _data(*shape)
    _, t0 = _ref(shape, kind)
    xd, dec = torch.from_numpy(x).cuda(), RF.Decoder(Hi)
    y = RF.fused(xd, t0, FS, dec)
    torch.cuda.synchronize()
    return xd, dec, t0, y


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3], SHAPES[1]], ids=IDS)
def test_guard_bands_every_element_written_and_poisoned_work(shape, monkeypatch):
    """y and the work space come from torch.empty: inside the guard both lie between 64 KiB bands of 0xFF and start out as 0xFF themselves.  The bands stay
    intact, every element of y is written by the call, and the poisoned work space gives the serial result bit for bit."""
    xd, dec, t0, y0 = _serial(shape)
    dec.on(xd.device)
    with GD.guard_outputs(monkeypatch) as g:
        y = RF.fused(xd, t0, FS, dec)
        assert len(g.bufs) == 2 and g.nbytes > y.numel() * 8           # y and the work space
        assert g.check(y) == 1
    assert ST.same_bits(y, y0)


def test_input_inside_a_nan_halo(monkeypatch):
    xd, dec, t0, y0 = _serial(SHAPES[1])
    xh = GD.haloed(xd.permute(3, 2, 1, 0).contiguous(), "nan").permute(3, 2, 1, 0)          # the memory order the wrapper hands over: no copy in between
    hh = GD.haloed(dec.on(xd.device), "nan")
    y = RF.fused(xh, t0, FS, RF.Decoder(dec.Hi, device_copy=hh))
    torch.cuda.synchronize()
    assert ST.same_bits(y, y0)


# ---------------------------------------------------------------------------------------------------------------- streams
def test_stream_delayed_producer_on_a_side_stream():
    """x and Hi are all-0xFF twins that receive the true data on a non-blocking side stream behind FILL_MS of fills; the call, issued at once on that stream,
    and a clone taken directly behind it give the serial result bit for bit, and the wrapper returns while the filler is still running (asynchronous on
    ``queue``: no synchronisation, no allocation through the device)"""
    shape = SHAPES[1]
    xd, dec, t0, y0 = _serial(shape)
    xm = xd.permute(3, 2, 1, 0).contiguous()                            # the memory order the wrapper hands over
    side = torch.cuda.Stream()
    fn = lambda xt, ht: RF.fused(xt.permute(3, 2, 1, 0), t0, FS, RF.Decoder(dec.Hi, device_copy=ht))
    with torch.cuda.stream(side):                                        # warm: allocator blocks of this stream, code objects
        fn(xm, dec.on(xd.device))
        fn(xm, dec.on(xd.device))
    torch.cuda.synchronize()
    (y,), (clone,), early = ST.run_delayed(fn, [xm, dec.on(xd.device)], side, FILL_MS)
    assert ST.same_bits(y, y0) and ST.same_bits(clone, y0)
    assert early, "the wrapper did not return before the queued work had run: it waits for the stream (or for the device)"


def test_stream_two_runs_are_bit_identical():
    """calls of different sizes issued alternately on two side streams behind a filler, against the same calls issued alone"""
    calls = []
    for shape in (SHAPES[0], SHAPES[3], SHAPES[1], SHAPES[2]):
        x, Hi = _data(*shape)
        xd, dec = torch.from_numpy(x).cuda(), RF.Decoder(Hi)
        dec.on(xd.device)
        calls.append(functools.partial(RF.fused, xd, T0, FS, dec))
    ST.interleaved(calls, torch.cuda.Stream(), torch.cuda.Stream(), FILL_MS * len(calls), reps=2)


def _churn(stream, nbytes, n=16):
    """on ``stream``: ``n`` allocations of ``nbytes`` filled with NaN bit patterns and held together, so that every free block of that size in the stream's pool
    is taken -- what the next uploads of a cache would do to a block the allocator has handed back to this stream's pool"""
    with torch.cuda.stream(stream):
        held = [torch.full((max(1, nbytes // 8),), float("nan"), dtype=torch.float64, device="cuda") for _ in range(n)]
    del held


def test_stream_cached_t0_hit_from_a_second_stream_then_evicted_from_the_first():
    """the per-pulse t0 table is uploaded by a call on stream A, hit by a call queued on stream B behind a filler, then evicted by calls on A with other
    tables (and A's pool churned with NaN): B's call must still read ITS table -- the cache records the consuming stream, so the block is not reused early"""
    shape = SHAPES[1]
    xd, dec, t0, y0 = _serial(shape, "per-pulse")
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(B):
        RF.fused(xd, t0 + 1e-7, FS, dec)                               # warm B's pool and code objects with another table
    with torch.cuda.stream(A):
        RF.fused(xd, t0, FS, dec)                                       # the table is built in A's pool
    torch.cuda.synchronize()
    ev = ST.filler(B, FILL_MS)
    with torch.cuda.stream(B):
        yB = RF.fused(xd, t0, FS, dec)                                  # a hit, queued behind the filler
    assert ST.returned_early(ev), "the hit waited for the stream: the case shows nothing"
    with torch.cuda.stream(A):
        for k in range(4):
            RF.fused(xd, t0 + (k + 2) * 1e-7, FS, dec)                  # evictions and same-sized uploads on A, which is idle: they run at once
    _churn(A, t0.nbytes)
    torch.cuda.synchronize()
    assert ST.same_bits(yB, y0)


def test_stream_decoder_dropped_while_a_second_stream_still_reads_it():
    """the same for the decoder's device copy: built on stream A, used by a call queued on B behind a filler, then the Decoder is dropped (what
    ``UltrasoundSystem.refocus`` does when its key changes) and A's pool is churned.  (Measured on an MI355X with ``record_stream`` made a no-op: the t0
    case above fails, this one still passed -- the allocator did not hand the dropped block to the churn in that run.  It guards the ordering; the t0 case
    is the one shown to catch the race.)"""
    shape = SHAPES[3]
    x, Hi = _data(*shape)
    xd, _, _, y0 = _serial(shape, "scalar")
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(B):
        RF.fused(xd, T0, FS, RF.Decoder(Hi))                           # warm
    dec = RF.Decoder(Hi)
    with torch.cuda.stream(A):
        nbytes = dec.on(xd.device).numel() * 8                          # the copy is built in A's pool
    torch.cuda.synchronize()
    ev = ST.filler(B, FILL_MS)
    with torch.cuda.stream(B):
        yB = RF.fused(xd, T0, FS, dec)
    assert ST.returned_early(ev), "the call waited for the stream: the case shows nothing"
    del dec
    _churn(A, nbytes)
    torch.cuda.synchronize()
    assert ST.same_bits(yB, y0)


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_end_to_end_greens_focustx_refocus_das():
    """reference test/BFTest.m:309-316 on the F2 PSF geometry of tests/golden (32 elements, scatterer at (2, 0, 15) mm): greens FSA data -> focusTx to 17
    plane waves -> zero-pad -> refocus -> FSA DAS; the image peaks within 1.1 mm of the scatterer in x and in z (the restatement alone meets this on the
    CPU: tests/test_refocus_host.py)"""
    c0, fc = 1500.0, 6e6
    fs = 4 * fc
    scat = np.array([2e-3, 0.0, 15e-3])
    xdc = Transducer.linear(32, 0.2e-3, fc)
    us = UltrasoundSystem(xdc, Sequence("FSA", c0=c0), Scan.cartesian(R.E2E_X, R.E2E_Z), fs=fs)
    t = np.arange(-2.0 / fc, 2.0 / fc, 1 / (4 * fs))
    wv = np.exp(-(t * fc * 1.2) ** 2) * np.exp(2j * np.pi * fc * t)
    fsa = us.greens(scat.reshape(3, 1), [1.0], wv, t[0], 4 * fs, R0=c0 / fc, focus=False)
    pw = Sequence("PW", R.pw_normals(R.E2E_ANGLES), c0)
    chd = us.focusTx(fsa, pw)
    assert tuple(chd.data.shape[1:3]) == (32, 17)
    chd = chd.zeropad(R.E2E_PAD, R.pad_behind(chd.T, RF.takes))
    assert RF.takes(chd.T)
    for method in ("adjoint", "tikhonov"):
        out, Hi = us.refocus(chd, pw, method=method)
        assert tuple(out.data.shape[:3]) == (chd.T, 32, 32) and out.data.dtype == torch.complex64 and Hi.shape == (32, 17, chd.T)
        assert out.t0 == float(np.min(chd.t0))
        b = us.DAS(out)
        torch.cuda.synchronize()
        img = b.abs().cpu().numpy().reshape(len(R.E2E_Z), len(R.E2E_X))
        assert img.max() > 0 and not np.isnan(img).any()
        iz, ix = np.unravel_index(np.argmax(img), img.shape)
        print(f"refocus end to end {method}: peak at x={R.E2E_X[ix] * 1e3:.3f} mm z={R.E2E_Z[iz] * 1e3:.3f} mm")
        assert abs(R.E2E_X[ix] - scat[0]) <= 1.1e-3 and abs(R.E2E_Z[iz] - scat[2]) <= 1.1e-3, (method, R.E2E_X[ix], R.E2E_Z[iz])
