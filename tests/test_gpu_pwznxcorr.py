"""pwznxcorr on the device (qdas_pwznxcorr, csrc/pwznxcorr.hip) against the float64 restatement of the reference's base-MATLAB branch
(tests/pwznxcorr_ref.py): options x precisions, windows and lags longer than the record, time tiles, every ``ref``, layouts passed in place
and copied, memory guards, DAS(keep_rx=True) end to end, bit-reproducibility.

Bound: max|got - ref| <= tol max|ref| with tol = 1e-5 (fp32) and 1e-12 (fp64), NaN where and only where the restatement has NaN."""
import numpy as np
import pytest

from tests import guards as GD
from tests import pwznxcorr_ref as R

pytestmark = pytest.mark.gpu


def _np(t):
    import torch
    return (t.to(torch.complex128) if t.is_complex() else t.to(torch.float64)).detach().cpu().numpy()


def _data(shape, cplx, seed, ndim_axis=1):
    """Gaussian noise with a gain in [1, 4] per channel (axis ``ndim_axis``)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if cplx else 0)
    g = [1] * len(shape)
    g[ndim_axis] = shape[ndim_axis]
    return x * (1 + 3 * rng.random(g))


def _bits(t):
    """the tensor's bit pattern as integers (NaN compares equal to itself)"""
    import torch
    t = t.contiguous()
    if t.is_complex():
        t = torch.view_as_real(t).contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _dtype(f64, cplx):
    import torch
    return {(False, False): torch.float32, (False, True): torch.complex64, (True, False): torch.float64, (True, True): torch.complex128}[(f64, cplx)]


def _dev(x, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(dt).cuda()


def _colmajor(x, dt):
    """device tensor of x's shape whose FIRST dimension is fastest (what DAS returns)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dt)
    rev = list(range(t.ndim - 1, -1, -1))
    return t.permute(rev).contiguous().cuda().permute(rev)


def _close(got, ref, f64, what=""):
    got = _np(got) if not isinstance(got, np.ndarray) else got
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN pattern differs"
    scale = np.nanmax(np.abs(ref)) if np.any(~np.isnan(ref)) else 1.0
    err = np.nanmax(np.abs(got - ref)) / scale if np.any(~np.isnan(ref)) else 0.0
    print(f"pwznxcorr {what}: rel err {err:.3e}")
    assert err <= (1e-12 if f64 else 1e-5), (what, err)


def _both(x, dt, lags, W=None, f64=False, what="", **kw):
    """x: numpy (time first); runs the column-major device tensor and compares with the restatement of the values the device saw"""
    from qups_amd import pwznxcorr
    xt = _colmajor(x, dt)
    y = pwznxcorr(xt, lags, W, **kw)
    assert y.dtype == dt and y.is_cuda
    kr = {k: v for k, v in kw.items() if k != "x0"}
    if "x0" in kw:
        kr["x0"] = _np(kw["x0"])
    _close(y, R.pwznxcorr(_np(xt), lags, W, **kr), f64, what)
    return y


# ---------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("pad", [True, False])
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("zero", [True, False])
@pytest.mark.parametrize("f64,cplx", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("W", [7, 8])
def test_options_and_precisions(W, f64, cplx, zero, norm, pad):
    x = _data((96, 5), cplx, seed=W + 2 * f64 + 4 * cplx)
    _both(x, _dtype(f64, cplx), 3, W, f64, f"W={W}", zero=zero, norm=norm, pad=pad)


@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("extra", [3, None])
def test_halo_across_time_tiles(extra, cplx):
    from qups_amd import correlator
    T = correlator.TIME_TILE + 3 if extra else 2 * correlator.TIME_TILE - 1
    x = _data((T, 3), cplx, seed=T)
    _both(x, _dtype(False, cplx), 6, 33, False, f"T={T}")


@pytest.mark.parametrize("zero", [True, False])
@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("W", [15, 16])
def test_middle_tiles_take_the_unmasked_window_loop(W, cplx, zero):
    """T >= 3 TIME_TILE: the tiles between the first and the last see no record end, so K(c) runs its unmasked loop (csrc/pwznxcorr.hip `interior`)"""
    from qups_amd import correlator
    T = 3 * correlator.TIME_TILE + 37
    assert T - 2 * correlator.TIME_TILE > 2 * W                  # a whole tile with its halo of 2 (W - 1) lies inside the record
    x = _data((T, 3), cplx, seed=W + cplx)
    _both(x, _dtype(False, cplx), 4, W, False, f"T={T} W={W} zero={zero}", zero=zero)
    if zero:
        _both(x, _dtype(True, cplx), [5, -2], W, True, f"T={T} W={W} f64", zero=zero, pad=False)


@pytest.mark.parametrize("pad", [True, False])
def test_window_longer_than_the_record(pad):
    _both(_data((40, 4), True, seed=40), _dtype(False, True), 3, 64, False, "T=40 W=64", pad=pad)
    _both(_data((40, 4), False, seed=41), _dtype(True, False), 3, 64, True, "T=40 W=64 f64", pad=pad)


@pytest.mark.parametrize("pad", [True, False])
def test_lag_longer_than_the_record(pad):
    _both(_data((8, 4), True, seed=8), _dtype(False, True), 10, 5, False, "T=8 L=10", pad=pad)
    _both(_data((8, 4), False, seed=9), _dtype(True, False), 10, None, True, "T=8 L=10 f64", pad=pad)


def test_the_stated_limit_in_complex_double():
    _both(_data((300, 3), True, seed=300), _dtype(True, True), 256, 256, True, "W=256 L=256")


def test_one_past_the_lds_limit_is_an_error_not_a_launch():
    import torch
    from qups_amd import _lib, correlator, pwznxcorr
    W = 256
    while correlator.lds_bytes(8, True, W, 512) <= correlator.LDS_LIMIT:
        W += 1
    assert correlator.lds_bytes(8, True, W - 1, 512) <= correlator.LDS_LIMIT < correlator.lds_bytes(8, True, W, 512)
    x = torch.zeros((300, 2), dtype=torch.complex128, device="cuda")
    with pytest.raises(_lib.QdasError, match="LDS") as e:
        pwznxcorr(x, 256, W, norm=False)
    assert e.value.code == _lib.QDAS_EUNSUPPORTED
    with pytest.raises(_lib.QdasError, match="lags"):
        pwznxcorr(x.real.to(torch.float32), np.zeros(correlator.MAX_LAGS + 1), 3)


def test_unsorted_and_duplicated_lags_stride_and_windows():
    x = _data((96, 6), True, seed=12)
    y = _both(x, _dtype(False, True), [3, -1, 3, 0], 9, False, "lags [3 -1 3 0]")
    import torch
    assert torch.equal(y[..., 0], y[..., 2])
    _both(x, _dtype(False, True), 3, 9, False, "stride 2", stride=2)
    hann = 0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(12) + 0.5) / 12)
    _both(x, _dtype(False, True), 3, hann, False, "hann")
    wz = np.array([1.0, 0.5, 0.0, 2.0, 0.0, 1.0])
    _both(x, _dtype(False, True), 3, wz, False, "zero weight")
    _both(x.real, _dtype(False, False), 3, np.ones(10) / 10, False, "mean window")


@pytest.mark.parametrize("N", [5, 6])
def test_center_reference(N):
    _both(_data((96, N), True, seed=N), _dtype(False, True), 3, 8, False, f"center N={N}", ref="center")
    _both(_data((96, N, 2), False, seed=N), _dtype(True, False), 3, 8, True, f"center N={N} batch", ref="center")


def test_x0_reference():
    x = _data((96, 5, 3), True, seed=20)
    dt = _dtype(False, True)
    one = _dev(_data((96, 1, 1), True, seed=21), dt)
    _both(x, dt, 3, 8, False, "x0 one trace", ref="x0", x0=one)
    full = _colmajor(_data((96, 5, 3), True, seed=22), dt)
    _both(x, dt, 3, 8, False, "x0 N x batch", ref="x0", x0=full)
    perb = _dev(_data((96, 1, 3), True, seed=23), dt)       # one trace per batch entry, row-major: copied with time fastest
    _both(x, dt, 3, 8, False, "x0 per batch", ref="x0", x0=perb)
    pern = _colmajor(_data((96, 5), True, seed=24), dt)
    _both(x, dt, 3, 8, False, "x0 per channel", ref="x0", x0=pern)


def test_an_all_zero_channel_gives_the_references_nan_pattern():
    x = _data((96, 5), True, seed=30)
    x[:, 2] = 0
    y = _both(x, _dtype(False, True), 3, 8, False, "zero channel")
    assert bool(y.isnan().any()) and not bool(y[:, 3].isnan().any())
    _both(x.real, _dtype(True, False), 3, 8, True, "zero channel f64")


# ---------------------------------------------------------------------------------------------------------------- layouts
def _spy(monkeypatch):
    """records, per call, (pointer of x as given, pointer _prepare returned, how, pointers of xl / xr handed to the launch)"""
    from qups_amd import correlator
    seen, prep, launch = [], correlator._prepare, correlator._launch

    def spy_prepare(x, x0, t, n):
        r = prep(x, x0, t, n)
        seen.append([x.data_ptr(), r[0].data_ptr(), r[3]])
        return r

    def spy_launch(xl, xr, *a, **k):
        seen[-1] += [xl.data_ptr(), xr.data_ptr()]
        return launch(xl, xr, *a, **k)
    monkeypatch.setattr(correlator, "_prepare", spy_prepare)
    monkeypatch.setattr(correlator, "_launch", spy_launch)
    return seen


def test_das_layout_is_read_in_place(monkeypatch):
    from qups_amd import pwznxcorr
    seen = _spy(monkeypatch)
    x = _data((96, 7, 4, 3), True, seed=50, ndim_axis=3)     # I1 x I2 x F x N, I1 fastest, N slowest
    xt = _colmajor(x, _dtype(False, True))
    y = pwznxcorr(xt, 2, 8, tdim=1, ndim=4)
    # the launch got x's own storage: the left traces at x, the right traces one channel stride further
    assert seen == [[xt.data_ptr(), xt.data_ptr(), "none", xt.data_ptr(), xt.data_ptr() + xt.stride(3) * xt.element_size()]], seen
    _close(y, R.pwznxcorr(_np(xt), 2, 8, tdim=1, ndim=4), False, "das layout")


def test_row_major_is_copied_once(monkeypatch):
    from qups_amd import pwznxcorr
    seen = _spy(monkeypatch)
    x = _data((96, 5), True, seed=51)
    xt = _dev(x, _dtype(False, True))                        # torch row-major T x N: the channels fastest
    y = pwznxcorr(xt, 3, 8)
    assert len(seen) == 1 and seen[0][2] == "copy" and seen[0][1] != xt.data_ptr() and seen[0][3] == seen[0][1]
    _close(y, R.pwznxcorr(_np(xt), 3, 8), False, "row major")


def test_time_second_channels_first(monkeypatch):
    from qups_amd import pwznxcorr
    seen = _spy(monkeypatch)
    x = _data((5, 96, 2), False, seed=52, ndim_axis=0)       # N x T x B row-major
    xt = _dev(x, _dtype(False, False))
    y = pwznxcorr(xt, 3, 8, tdim=2, ndim=1)
    _close(y, R.pwznxcorr(x, 3, 8, tdim=2, ndim=1), False, "tdim=2 ndim=1")
    xt2 = _dev(x.transpose(2, 0, 1), _dtype(False, False)).permute(1, 2, 0)   # the same values with time fastest: in place
    y2 = pwznxcorr(xt2, 3, 8, tdim=2, ndim=1)
    assert seen[1][2] == "none" and seen[1][3] == xt2.data_ptr()
    import torch
    assert torch.equal(y, y2)


def test_two_batch_dimensions_and_the_lag_dimension_in_the_middle():
    from qups_amd import pwznxcorr
    x = _data((96, 4, 3, 2), True, seed=53)
    _both(x, _dtype(False, True), 2, 8, False, "4-D")
    big = _colmajor(_data((96, 4, 5, 2), True, seed=54), _dtype(False, True))
    xt = big[:, :, ::2]                                      # two batch groups that do not merge
    _close(pwznxcorr(xt, 2, 8), R.pwznxcorr(_np(xt), 2, 8), False, "two groups")
    x5 = _data((96, 4, 1, 3), False, seed=55)
    xt5 = _colmajor(x5, _dtype(False, False))
    y = pwznxcorr(xt5, 2, 8, ldim=3)
    assert tuple(y.shape) == (96, 3, 5, 3)
    _close(y, R.pwznxcorr(x5, 2, 8, ldim=3), False, "ldim=3")
    y = pwznxcorr(xt5, 2, 8, ldim=6)
    assert tuple(y.shape) == (96, 3, 1, 3, 1, 5)
    _close(y, R.pwznxcorr(x5, 2, 8, ldim=6), False, "ldim=6")


def test_half_precision_is_upcast_and_cast_back():
    import torch
    from qups_amd import pwznxcorr
    x = _data((96, 5), False, seed=56)
    xt = _colmajor(x, torch.float16)
    y = pwznxcorr(xt, 3, 8)
    assert y.dtype == torch.float16 and tuple(y.shape) == (96, 4, 7)
    ref = R.pwznxcorr(_np(xt), 3, 8)
    assert np.abs(_np(y) - ref).max() <= (2.0 ** -11 + 1e-5) * np.abs(ref).max()   # (the cast back to half rounds to 2^-11 of the value)
    zt = _colmajor(_data((96, 5), True, seed=57), torch.complex64).to(torch.complex32)
    z = pwznxcorr(zt, 3, 8)
    assert z.dtype == torch.complex32 and tuple(z.shape) == (96, 4, 7)
    zin = torch.view_as_real(zt).float().cpu().numpy()
    ref = R.pwznxcorr(zin[..., 0] + 1j * zin[..., 1], 3, 8)
    zout = torch.view_as_real(z).float().cpu().numpy()
    # each component is rounded to half: 2^-11 of the component, at most 2^-11 sqrt(2) of the maximum modulus
    assert np.abs(zout[..., 0] + 1j * zout[..., 1] - ref).max() <= (2.0 ** -10.5 + 1e-5) * np.abs(ref).max()


# ---------------------------------------------------------------------------------------------------------------- other checks
def test_two_runs_are_bit_identical():
    import torch
    from qups_amd import pwznxcorr
    xt = _colmajor(_data((600, 9, 3), True, seed=60), _dtype(False, True))
    a, b = pwznxcorr(xt, 4, 16), pwznxcorr(xt, 4, 16)
    assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("layout", ["in place", "copied"])
def test_guard_bands_and_unwritten_outputs(layout, monkeypatch):
    import torch
    from qups_amd import pwznxcorr
    x = _data((300, 5, 2), True, seed=61)
    dt = _dtype(False, True)
    xt = _colmajor(x, dt) if layout == "in place" else _dev(x, dt)
    run = lambda: pwznxcorr(xt, [2, -3, 0], 9)
    r0 = run()
    torch.cuda.synchronize()
    del r0
    with GD.guard_outputs(monkeypatch) as g:
        y = run()
        assert g.check(y) >= 1, "the result aliases no guarded buffer"
    _close(y, R.pwznxcorr(_np(xt), [2, -3, 0], 9), False, f"guarded, {layout}")


@pytest.mark.parametrize("layout", ["in place", "strided view", "copied"])
def test_poisoned_halo(layout):
    import torch
    from qups_amd import pwznxcorr
    x = _data((300, 5, 2), True, seed=62)
    dt = _dtype(False, True)
    if layout == "in place":
        xt = _colmajor(x, dt)
        halo = lambda f: GD.haloed_view(xt, f)
    elif layout == "copied":                                 # row-major, channels fastest: the copy and the kernel behind it see only x
        xt = _dev(x, dt)
        halo = lambda f: GD.haloed(xt, f)
    else:                                                    # every second channel of a wider buffer: the skipped records are poisoned too
        big = _colmajor(_data((300, 10, 2), True, seed=63), dt)
        xt = big[:, ::2]
        halo = lambda f: GD.haloed_view(xt, f)
    outs = [pwznxcorr(halo(f), 3, 9) for f in (0, "nan", "inf")]
    torch.cuda.synchronize()
    assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(_bits(outs[0]), _bits(outs[2])), "the result depends on what surrounds its input"
    _close(outs[0], R.pwznxcorr(_np(xt), 3, 9), False, f"halo, {layout}")


def test_greens_das_keep_rx_end_to_end(monkeypatch):
    """greens -> DAS(keep_rx=True) on a tiny scan -> pwznxcorr along depth across receivers, against the restatement of the same tensor"""
    import torch
    from qups_amd import Scan, Sequence, Transducer, UltrasoundSystem, pwznxcorr
    fc, c0 = 5e6, 1500.0
    fs = 4 * fc
    xdc = Transducer.linear(16, 0.3e-3, fc)
    us = UltrasoundSystem(xdc, Sequence("FSA", c0=c0), Scan.cartesian(np.linspace(-2e-3, 2e-3, 9), np.linspace(8e-3, 12e-3, 70)), fs=fs)
    t = np.arange(-2.0 / fc, 2.0 / fc, 1 / (4 * fs))
    wv = np.exp(-(t * fc * 1.2) ** 2) * np.exp(2j * np.pi * fc * t)
    rng = np.random.default_rng(31)
    scat = np.stack([rng.uniform(-2e-3, 2e-3, 40), np.zeros(40), rng.uniform(8e-3, 12e-3, 40)])
    chd = us.greens(scat, rng.uniform(0.5, 1.5, 40), wv, t[0], 4 * fs, R0=c0 / fc)
    b = us.DAS(chd, interp="linear", keep_rx=True)           # I1 x I2 x I3 x F x N x 1, depth fastest
    assert b.is_cuda and b.shape[0] == 70 and int(torch.count_nonzero(b)) > b.numel() // 2
    rx = list(b.shape).index(16)
    seen = _spy(monkeypatch)
    y = pwznxcorr(b, 2, 6, tdim=1, ndim=rx + 1)
    assert seen == [[b.data_ptr(), b.data_ptr(), "none", b.data_ptr(), b.data_ptr() + b.stride(rx) * b.element_size()]], seen
    assert y.shape[rx] == 15 and y.shape[-1] == 5 and y.shape[0] == 70
    assert not bool(y.isnan().all())
    _close(y, R.pwznxcorr(_np(b), 2, 6, tdim=1, ndim=rx + 1), False, "greens -> DAS keep_rx")
