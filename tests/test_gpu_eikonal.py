"""The eikonal solver, the table sampler and ``bfEikonal`` on the device against the float64 oracle of tests/eikonal_ref.py.

Maps: ``max |T_gpu - T_ref| <= 1e-9 dp / max(c)`` over EVERY node.  Both sides solve the same discrete system in fp64, so only rounding separates
them; the square root is well conditioned where it is used (the two-neighbour branch holds for ``|a - b| < s``, where the discriminant is
``>= s^2``).  Three CPU solvers of that system agree to 1.2e-13 of a cell's travel time; 1e-9 leaves four decades."""
import numpy as np
import pytest

from tests import eikonal_ref as R

pytestmark = pytest.mark.gpu

DP = 0.25e-3


def _np(t):
    return t.detach().cpu().numpy()


def _check_maps(c, dp, sets, T):
    """every node of every map against the oracle; prints the largest deviation in cells"""
    bound = 1e-9 * dp / np.max(c)
    worst = 0.0
    for k, s in enumerate(sets):
        ref = R.fmm(c, dp, s)
        err = np.abs(_np(T[:, :, k]) - ref).max()
        worst = max(worst, err)
        print(f"map {k}: max |T - ref| = {err / (dp / np.max(c)):.3e} cell")
        assert np.all(np.isfinite(_np(T[:, :, k]))) and err <= bound, (k, err, bound)
    return worst


def _solve(c, dp, sets, **kw):
    from qups_amd import eikonal as E
    return E.eikonal(c, dp, [np.asarray(s, float).reshape(2, -1) for s in sets], **kw)


PLACES = lambda C1, C2: [[[1.0], [1.0]], [[C1], [1.0]], [[1.0], [C2]], [[C1], [C2]],                       # corners
                         [[1.0], [C2 / 2 + 0.37]], [[C1], [C2 / 3 + 0.9]], [[C1 / 2 + 0.6], [1.0]], [[C1 / 3 + 0.2], [C2]],   # edges
                         [[C1 / 2 + 0.45], [C2 / 2 + 0.8]], [[0.7 * C1 + 0.99], [0.2 * C2 + 1.01]]]          # inside, fractional


def test_homogeneous_every_source_place():
    C1, C2 = 61, 45
    c = np.full((C1, C2), 1540.0)
    sets = PLACES(C1, C2)
    _check_maps(c, DP, sets, _solve(c, DP, sets))


def test_layers_and_disc_and_a_multi_point_set():
    from qups_amd import eikonal as E
    c = R.layers_disc(161, 121)
    sets = [[[1.0], [61.0]], [[1.4], [3.9]], [[30.2, 100.7, 161.0], [10.5, 60.1, 121.0]]]
    T = _solve(c, DP, sets)
    _check_maps(c, DP, sets, T)
    assert 0 < E.last_passes() <= E.pass_cap(161, 121)
    print("passes", E.last_passes(), "cap", E.pass_cap(161, 121))


def test_smooth_random_map():
    c = R.smooth_random(97, 139, seed=5)
    assert c.max() / c.min() <= 2
    sets = [[[48.3], [70.2]], [[1.0], [139.0]], [[97.0], [20.6]]]
    _check_maps(c, DP, sets, _solve(c, DP, sets))


@pytest.mark.parametrize("shape", [(2, 37), (3, 3), (37, 2), (3, 50), (16, 16), (16, 48), (48, 16), (17, 33), (1, 40), (40, 1), (15, 31), (2, 2)])
def test_odd_grid_shapes(shape):
    """sides that are not multiples of the tile, exactly one tile, 1 x n and n x 1 tiles' worth, sides of 1, 2 and 3 nodes"""
    C1, C2 = shape
    c = R.smooth_random(C1, C2, seed=C1 + 100 * C2)
    sets = [[[1.0], [1.0]], [[C1], [C2]], [[min((C1 + 1) / 2 + 0.25, C1)], [min((C2 + 1) / 2 + 0.25, C2)]]]
    _check_maps(c, DP, sets, _solve(c, DP, sets))


def test_64_sources_in_one_call_equal_one_per_call():
    C1, C2 = 70, 90
    c = R.layers_disc(C1, C2)
    rng = np.random.default_rng(2)
    src = np.stack([rng.uniform(1, C1, 64), rng.uniform(1, C2, 64)])
    T = _np(_solve(c, DP, [src[:, k:k + 1] for k in range(64)]))
    bound = 1e-9 * DP / c.max()
    worst = 0.0
    for k in range(64):
        one = _np(_solve(c, DP, [src[:, k:k + 1]]))[:, :, 0]
        worst = max(worst, np.abs(one - T[:, :, k]).max())
    print(f"batched vs single: {worst / (DP / c.max()):.3e} cell")
    assert worst <= bound
    _check_maps(c, DP, [src[:, k:k + 1] for k in (0, 31, 63)], _solve(c, DP, [src[:, k:k + 1] for k in (0, 31, 63)]))


def test_contrast_ten_to_one_converges_under_the_cap():
    """head waves along a 10 : 1 interface: tiles are revisited many times, the solve must still end under the derived cap"""
    from qups_amd import eikonal as E
    C1, C2 = 120, 150
    c = np.full((C1, C2), 1000.0)
    c[60:] = 10000.0
    sets = [[[5.0], [8.0]], [[118.2], [140.0]], [[60.0], [75.0]]]
    T = _solve(c, DP, sets)
    print("passes", E.last_passes(), "cap", E.pass_cap(C1, C2))
    assert E.last_passes() <= E.pass_cap(C1, C2)
    _check_maps(c, DP, sets, T)


def test_the_pass_cap_is_an_error_and_no_map():
    """max_passes = 1 on a solve that needs more: an ordinary error return (QDAS_ENOCONV), nothing hangs, no unconverged map comes back"""
    from qups_amd import _lib
    from qups_amd import eikonal as E
    c = np.full((80, 80), 1500.0)
    with pytest.raises(_lib.QdasError) as ei:
        _solve(c, DP, [[[1.0], [1.0]]], max_passes=1)
    assert ei.value.code == _lib.QDAS_ENOCONV and "no fixed point within 1 passes" in ei.value.message
    assert E.last_passes() == 1
    # ... and no map: a direct call into a tensor the test owns leaves NaN at every node, not the unconverged values
    import ctypes as C
    import torch
    cc = torch.full((80, 80), 1500.0, dtype=torch.float64, device="cuda")
    T0 = torch.zeros((80, 80), dtype=torch.float64, device="cuda")
    src = np.array([[1.0, 1.0]])
    d = _lib.EikonalDesc()
    d.C1, d.C2, d.K, d.npts, d.dp, d.base, d.max_passes, d.device = 80, 80, 1, 1, DP, 1, 1, -1
    rc = _lib.lib().qdas_eikonal(C.byref(d), C.c_void_p(cc.data_ptr()), C.c_void_p(src.ctypes.data), C.c_void_p(T0.data_ptr()),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.QDAS_ENOCONV and bool(torch.isnan(T0).all())
    T = _solve(c, DP, [[[1.0], [1.0]]])                       # the default cap: converges, and the library is as usable as before
    assert np.isfinite(_np(T)).all() and E.last_passes() > 1
    one = _solve(np.full((10, 10), 1500.0), DP, [[[3.0], [3.0]]], max_passes=2)    # a one-tile grid needs one pass and one that finds nothing to do
    assert np.isfinite(_np(one)).all() and E.last_passes() <= 2


def test_msfm_contract():
    """speed in cells per second, 1-based floored points, several points -> one map"""
    from qups_amd import msfm
    F = R.smooth_random(40, 30, seed=9) / DP
    sp = np.array([[3.7, 30.2], [4.1, 22.9]])
    T = _np(msfm(F, sp))
    ref = R.fmm(F, 1.0, sp)
    assert T.shape == (40, 30) and T[2, 3] == 0 and T[29, 21] == 0
    assert np.abs(T - ref).max() <= 1e-9 / F.max()


# ---------------------------------------------------------------------------------------------------------------- tables
def _system(nel=8, x=None, z=None, pitch=0.3e-3, rx=None):
    from qups_amd import Scan, Sequence, Transducer, UltrasoundSystem
    xdc = Transducer.linear(nel, pitch)
    scan = Scan.cartesian(np.linspace(-3e-3, 3e-3, 49) if x is None else x, np.linspace(0, 8e-3, 65) if z is None else z)
    return UltrasoundSystem(xdc, Sequence("FSA", c0=1500.0), scan, rx=rx)


def _cmap(us, cgrd=None):
    from qups_amd import eikonal as E
    _, _, _, _, size = E.scan_grid(cgrd or us.scan)
    c = R.layers_disc(*size)
    return c.reshape((cgrd or us.scan).size)


def _oracle_tables(us, c, cgrd):
    """the oracle's maps of the oracle's sampler, through the package's coordinate mapping"""
    from qups_amd import eikonal as E
    og, dp, dims, axes, size = E.scan_grid(cgrd)
    c2 = np.asarray(c, float).reshape(size)
    Pi = E.grid_coordinates(np.asarray(us.scan.positions()).reshape(3, -1, order="F"), og, dp, axes)
    out = []
    for xd in (us.rx, us.tx):
        g = E.grid_coordinates(xd.positions(), og, dp, axes)
        maps = [R.fmm(c2, dp, g[:, n:n + 1]) for n in range(g.shape[1])]
        out.append((np.stack([R.sample(m, Pi).reshape(us.scan.size, order="F") for m in maps], -1), maps))
    return out[0][0], out[1][0], out[0][1], dp, c2


def test_tables_on_the_grid_itself_are_the_maps():
    us = _system()
    c = _cmap(us)
    _, tau_rx, tau_tx = us.bfEikonal(None, c, delay_only=True)
    ref_rx, _, maps, dp, c2 = _oracle_tables(us, c, us.scan)
    assert tuple(tau_rx.shape) == us.scan.size + (8,) and tuple(tau_tx.shape) == us.scan.size + (1, 8)
    from qups_amd import eikonal as E
    og, dpp, dims, axes, size = E.scan_grid(us.scan)
    Tg = _np(E.eikonal(c2, dp, E.grid_coordinates(us.rx.positions(), og, dp, axes)))
    a = _np(tau_rx)[:, :, 0, :]
    assert np.all(np.abs(a - Tg) <= 1e-12 * np.abs(Tg))                       # scan == cgrd: table n IS map n at every pixel
    assert np.abs(a - np.stack(maps, -1)).max() <= 1e-9 * dp / c2.max()


def test_tables_of_a_finer_offset_scan_and_nan_outside():
    from qups_amd import Scan
    cgrd = Scan.cartesian(np.linspace(-2.5e-3, 2.5e-3, 41), np.linspace(0, 7e-3, 57))            # step 0.125 mm
    us = _system(x=np.linspace(-3e-3, 3e-3, 97) + 0.013e-3, z=np.linspace(-0.2e-3, 7.4e-3, 153), pitch=0.25e-3)   # finer, offset, and larger than the grid
    c = _cmap(us, cgrd)
    b0, tau_rx, tau_tx = us.bfEikonal(None, c, cgrd, delay_only=True, keep_rx=True)
    assert tuple(b0.shape) == us.scan.size + (8, 1, 0)
    ref_rx, ref_tx, maps, dp, c2 = _oracle_tables(us, c, cgrd)
    a = _np(tau_rx)
    assert np.array_equal(np.isnan(a), np.isnan(ref_rx)) and np.isnan(a).any() and not np.isnan(a).all()
    ok = ~np.isnan(ref_rx)
    err = np.abs(a[ok] - ref_rx[ok])
    print(f"tables: max err {err.max() / (dp / c2.max()):.3e} cell")
    assert np.all(err <= 1e-9 * dp / c2.max() + 1e-12 * np.abs(ref_rx[ok]))
    assert np.array_equal(_np(tau_tx)[:, :, :, 0, :], a, equal_nan=True)      # tx is rx: the same tables


# ---------------------------------------------------------------------------------------------------------------- images
def _chd(us, prec, seed=0, T=420, fs=25e6):
    import torch
    from qups_amd import ChannelData
    rng = np.random.default_rng(seed)
    N, M = us.rx.numel, us.tx.numel
    x = (rng.standard_normal((T, N, M)) + 1j * rng.standard_normal((T, N, M)))
    x = x.astype(np.complex64 if prec == "single" else np.complex128)
    return ChannelData(torch.from_numpy(x), 0.0, fs)


def rel_err(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("interp", ["linear", "cubic", "lanczos3"])
@pytest.mark.parametrize("keep,fmod,apod,prec", [("sum", 0.0, False, "single"), ("rx", 0.0, False, "single"), ("tx", 2e6, False, "single"),
                                                 ("sum", 2e6, True, "single"), ("sum", 0.0, False, "double"), ("rx", 2e6, True, "double")])
def test_bfEikonal_image_against_bfDASLUT_of_the_oracle_tables(interp, keep, fmod, apod, prec):
    """the same consumer with the oracle's tables; tolerances: those of the das_lut-versus-oracle tests of tests/test_gpu_golden.py (1e-4 single on the
    fused and generic kernels, 1e-9 double).  'nearest' is left out: a tap can flip on a rounding-level delay difference."""
    from qups_amd import Scan
    cgrd = Scan.cartesian(np.linspace(-2.5e-3, 2.5e-3, 41), np.linspace(0, 7e-3, 57))
    us = _system(x=np.linspace(-2.4e-3, 2.4e-3, 33), z=np.linspace(0.1e-3, 6.9e-3, 120))
    c = _cmap(us, cgrd)
    chd = _chd(us, prec)
    kw = dict(fmod=fmod, interp=interp, keep_rx=keep == "rx", keep_tx=keep == "tx", prec=prec)
    if apod:
        kw["apod"] = np.random.default_rng(4).uniform(0.2, 1.0, us.scan.size + (8, 1))
    b = _np(us.bfEikonal(chd, c, cgrd, **kw))
    ref_rx, ref_tx, _, _, _ = _oracle_tables(us, c, cgrd)
    ref = _np(us.bfDASLUT(chd, ref_rx, ref_tx, **kw))
    err = rel_err(b, ref)
    print(f"{interp} {keep} {prec}: rel err {err:.3e}")
    assert b.shape == ref.shape and np.abs(ref).max() > 0
    assert err <= (1e-4 if prec == "single" else 1e-9)


@pytest.mark.parametrize("prec", ["single", "double"])
def test_pixels_outside_the_grid_are_nan_in_the_table_and_zero_in_the_image(prec):
    from qups_amd import Scan
    cgrd = Scan.cartesian(np.linspace(-1.5e-3, 1.5e-3, 25), np.linspace(0, 6e-3, 49))
    us = _system(nel=32, x=np.linspace(-3e-3, 3e-3, 49), z=np.linspace(0.0, 8e-3, 129), pitch=0.09e-3)
    chd = _chd(us, prec, T=300)
    b, tau_rx, tau_tx = us.bfEikonal(chd, 1500.0, cgrd, return_delays=True, prec=prec)
    out = np.isnan(_np(tau_rx)).all(-1)
    assert out.any() and not out.all()
    assert np.array_equal(np.isnan(_np(tau_rx)).any(-1), out)               # a pixel is outside for every element or for none
    img = _np(b).reshape(us.scan.size)
    assert np.all(img[out] == 0) and np.all(np.isfinite(img)) and np.abs(img[~out]).min() > 0
    ref_rx, ref_tx, _, _, _ = _oracle_tables(us, np.full(cgrd.size, 1500.0), cgrd)
    ref = _np(us.bfDASLUT(chd, ref_rx, ref_tx, prec=prec)).reshape(us.scan.size)
    assert rel_err(img, ref) <= (1e-4 if prec == "single" else 1e-9)


def test_homogeneous_and_tx_is_rx_share_the_tables():
    from qups_amd import Transducer
    us = _system()
    _, tau_rx, tau_tx = us.bfEikonal(None, 1540.0, delay_only=True)
    assert tau_tx.data_ptr() == tau_rx.data_ptr()                             # the same storage
    us2 = _system(rx=Transducer.linear(8, 0.25e-3))                           # another receive aperture: tables of their own
    _, r2, t2 = us2.bfEikonal(None, 1540.0, delay_only=True)
    assert t2.data_ptr() != r2.data_ptr() and np.array_equal(_np(t2)[:, :, :, 0, :], _np(tau_rx))


def test_sources_are_solved_in_blocks_under_a_map_budget():
    from qups_amd import eikonal as E
    c = R.layers_disc(50, 40)
    src = np.stack([np.linspace(1, 50, 9), np.linspace(1.5, 39.5, 9)])
    i, j = np.meshgrid(np.arange(50) + 1.0, np.arange(40) + 1.0, indexing="ij")
    Pi = np.stack([i.ravel(order="F"), j.ravel(order="F")])
    full = _np(E.travel_time_tables(c, DP, src, Pi, (50, 40, 1)))
    blocked = _np(E.travel_time_tables(c, DP, src, Pi, (50, 40, 1), budget=2 * 50 * 40 * 8))     # two maps at a time
    assert full.shape == (50, 40, 1, 9) and np.array_equal(full, blocked)
