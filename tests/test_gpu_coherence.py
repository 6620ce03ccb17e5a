"""slsc / dmas / cohfac / pcf on the device (qdas_coherence, csrc/coherence.hip) against the float64 restatement of the reference's MATLAB
branches (tests/coherence_ref.py): every estimator x {f32, f64} x {real, complex} x layouts, awkward sizes and lag sets, DAS(keep_rx=True)
end to end without a copy of its output, bit-reproducibility."""
import numpy as np
import pytest

from tests import coherence_ref as R

pytestmark = pytest.mark.gpu

METHODS = ["average", "ensemble", "dmas", "cohfac", "pcf"]


def _np(t):
    return t.detach().cpu().numpy()


def _data(shape, cplx, seed, nan=False, zero_px=False):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if cplx else 0)
    x = x * (1 + 3 * rng.random(shape[:-1] + (1,)))
    if nan:
        x.reshape(-1)[rng.integers(0, x.size, 3)] = np.nan
    if zero_px:
        x[0, 0, ...] = 0
    return x


def _layout(x, dt, layout):
    """x: numpy I1 x I2 x N (or I1 x I2 x K x N); returns a device tensor of that shape in the given layout"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dt)
    nd = t.ndim
    if layout == "das":                                      # column-major: I1 fastest, N slowest (what DAS returns)
        return t.permute(*range(nd - 1, -1, -1)).contiguous().cuda().permute(*range(nd - 1, -1, -1))
    if layout == "aperture":                                 # torch row-major ... x N: the aperture fastest
        return t.contiguous().cuda()
    if layout == "odd":                                      # every second I1 of a wider column-major buffer
        big = torch.zeros((2 * x.shape[0],) + tuple(x.shape[1:]), dtype=dt)
        big[::2] = t
        bb = big.permute(*range(nd - 1, -1, -1)).contiguous().cuda().permute(*range(nd - 1, -1, -1))
        return bb[::2]
    raise ValueError(layout)


def _run(method, xt, dim, L=None, kdim=None):
    from qups_amd import coherence as Q
    if method in ("average", "ensemble"):
        return Q.slsc(xt, dim, L, method, kdim)
    if method == "dmas":
        return Q.dmas(xt, dim, L)
    if method == "cohfac":
        return Q.cohfac(xt, dim if kdim is None else [dim, kdim])
    return Q.pcf(xt, dim)


def _ref(method, x, axis, L=None, kaxis=None):
    if method in ("average", "ensemble"):
        return R.slsc(x, axis, L, method, kaxis)
    if method == "dmas":
        return R.dmas(x, axis, L)
    if method == "cohfac":
        return R.cohfac(x, axis if kaxis is None else (axis, kaxis))
    return R.pcf(x, axis)


def _check(method, y, x, axis, L=None, kaxis=None, f64=False):
    ref = _ref(method, x, axis, L, kaxis)
    tol = 1e-12 if f64 else 1e-5
    if method == "dmas":
        b = _np(y).astype(np.complex128)
        scale = R.dmas_pairs_abs(x, axis)
        got = b * np.abs(b)
        bad = ~(np.abs(got - ref) <= (1e-12 if f64 else 2e-5) * scale + 1e-300)
        assert not np.any(bad & ~(np.isnan(got) & np.isnan(ref))), float(np.nanmax(np.abs(got - ref) / np.maximum(scale, 1e-300)))
        return
    if method == "pcf":
        w, sf = y
        np.testing.assert_allclose(_np(w), ref[0], atol=tol, rtol=0)
        np.testing.assert_allclose(_np(sf), ref[1], atol=tol * 10, rtol=0)
        return
    got = _np(y)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    np.testing.assert_allclose(got, ref, atol=tol, rtol=0)


@pytest.mark.parametrize("layout", ["das", "aperture", "odd"])
@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("method,cplx", [(m, c) for m in METHODS for c in (True, False) if m != "pcf" or c])   # (pcf: complex input only)
def test_estimators_match_the_restatement(method, f64, cplx, layout):
    import torch
    x = _data((37, 3, 24), cplx, seed=sum(map(ord, f"{method}{f64}{cplx}{layout}")), zero_px=True)   # 111 pixels: not a multiple of 64
    dt = {(False, False): torch.float32, (False, True): torch.complex64, (True, False): torch.float64, (True, True): torch.complex128}[(f64, cplx)]
    xt = _layout(x, dt, layout)
    y = _run(method, xt, 3)
    x_used = _np(xt).astype(np.complex128 if cplx else np.float64)
    _check(method, y, x_used, 2, f64=f64)


@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("method", ["average", "ensemble", "cohfac"])
def test_time_kernel_dimension(method, cplx):
    import torch
    x = _data((29, 4, 5, 16), cplx, seed=5)                   # I1 x I2 x K x N
    xt = _layout(x, torch.complex64 if cplx else torch.float32, "das")
    y = _run(method, xt, 4, kdim=3)
    _check(method, y, _np(xt).astype(np.complex128 if cplx else np.float64), 3, kaxis=2)


@pytest.mark.parametrize("N", [1, 2, 7, 128, 1000])
@pytest.mark.parametrize("method", METHODS)
def test_aperture_sizes(method, N):
    import torch
    x = _data((70, 1, N), True, seed=N)
    xt = _layout(x, torch.complex64, "das")
    _check(method, _run(method, xt, 3), _np(xt).astype(np.complex128), 2)


@pytest.mark.parametrize("L", [[0, 5], [3, 3, 9], [2, 40, 41, 90], 100, [0, 0], [1, 7, 30], [0, 1, 2]])
@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("method", ["average", "ensemble", "dmas"])
def test_lag_sets(method, cplx, L):
    """lag 0, duplicates, lags >= N, scalars beyond N, sparse tables; N = 80 puts lags in chunks past the first (l0 > 0: the two-load path)"""
    import torch
    x = _data((50, 2, 80), cplx, seed=3)
    dts = ((torch.complex64, False), (torch.complex128, True)) if cplx else ((torch.float32, False), (torch.float64, True))
    for dt, f64 in dts:
        xt = _layout(x, dt, "das")
        _check(method, _run(method, xt, 3, L), _np(xt).astype(np.complex128 if cplx else np.float64), 2, L=L, f64=f64)


def test_lag_zero_is_three_quarters_on_the_device():
    import torch
    from qups_amd import slsc
    x = torch.full((64, 20), 1.5 * np.exp(0.7j), dtype=torch.complex64, device="cuda")
    z = _np(slsc(x, 2, [0, 5]))
    np.testing.assert_allclose(z.real, 0.75, atol=1e-6)


@pytest.mark.parametrize("method", METHODS)
def test_nan_samples(method):
    import torch
    x = _data((45, 2, 16), True, seed=11, nan=True)
    xt = _layout(x, torch.complex64, "das")
    y = _run(method, xt, 3)
    ref = _ref(method, x, 2)
    if method == "dmas":
        assert np.array_equal(np.isnan(_np(y)), np.isnan(ref))
    _check(method, y, x, 2)


def test_pcf_small_phase_spread():
    import torch
    from qups_amd import pcf
    rng = np.random.default_rng(0)
    N = 128
    ph = np.array([0.3, np.pi - 2e-3, -2.0])[:, None] + 1e-3 * rng.standard_normal((3, N))
    ph = np.where(ph > np.pi, ph - 2 * np.pi, ph)
    x = 2.0 * np.exp(1j * ph)
    w, sf = pcf(torch.from_numpy(x).to(torch.complex64).cuda(), 2)
    rw, rsf = R.pcf(_np(torch.from_numpy(x).to(torch.complex64)), 1)
    np.testing.assert_allclose(_np(sf), rsf, rtol=1e-3)
    np.testing.assert_allclose(_np(w), rw, atol=1e-5)


def test_half_precision_is_upcast_and_cast_back():
    import torch
    from qups_amd import cohfac, slsc
    x = _data((40, 2, 12), True, seed=9)
    xt = torch.from_numpy(x).to(torch.complex64).to(torch.complex32).cuda()
    z = slsc(xt, 3)
    assert z.dtype == torch.complex32 and tuple(z.shape) == (40, 2, 1)
    r = cohfac(xt, 3)
    assert r.dtype == torch.float16


def test_das_keep_rx_end_to_end_without_a_copy(monkeypatch):
    import torch
    from qups_amd import ChannelData, Scan, Sequence, Transducer, UltrasoundSystem, coherence
    from tests.cases import make_case
    case = make_case(seq="FSA", interp="linear", seed=31, N=16, I1=70, I2=9)
    xdc = Transducer(case["Pr"], np.stack([0 * case["Pr"][0], 0 * case["Pr"][0], 1 + 0 * case["Pr"][0]]))
    us = UltrasoundSystem(xdc, Sequence("FSA", focus=case["Nv"], c0=case["c"]), Scan(case["Pi"]))
    chd = ChannelData(torch.from_numpy(case["x"]), case["t0"], case["fs"])
    b = us.DAS(chd, interp="linear", keep_rx=True)
    rx = list(b.shape).index(16)                              # I1 x I2 x I3 x F x N x 1 (the summed transmit dimension stays)
    assert b.is_cuda and b.ndim - rx == 2
    seen = []
    orig = coherence._to_canonical

    def spy(x, reduced):
        t, how = orig(x, reduced)
        seen.append((t.data_ptr(), how))
        return t, how
    monkeypatch.setattr(coherence, "_to_canonical", spy)
    bn = _np(b).astype(np.complex128)
    dim = rx + 1
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    for method in METHODS:
        y = _run(method, b, dim)
        _check(method, y, bn, dim - 1)
    out_bytes = 2 * b.numel() // b.shape[-1] * b.element_size()
    assert torch.cuda.max_memory_allocated() - base <= 4 * out_bytes + (1 << 20)
    assert seen and all(p == b.data_ptr() and how == "none" for p, how in seen), seen


@pytest.mark.parametrize("method", METHODS)
def test_two_calls_are_bit_identical(method):
    import torch
    x = _data((300, 3, 64), True, seed=2)
    xt = _layout(x, torch.complex64, "das")
    a, b = _run(method, xt, 3), _run(method, xt, 3)
    if method == "pcf":
        assert all(torch.equal(u, v) for u, v in zip(a, b))
    else:
        assert torch.equal(a, b)
