"""The 3-D eikonal solver (csrc/eikonal3.hip), its table sampler and the volume path of ``bfEikonal`` on the device against the float64 oracle of
tests/eikonal3_ref.py: heap fast marching with msfm3d's rule, and the sampler's restatement.

Maps: ``max |T_gpu - T_ref| <= 1e-9 dp / max(c)`` over EVERY node -- the bound of tests/test_gpu_eikonal.py.  Both sides solve the same discrete system in
fp64 (the device as the fixed point of the classical upwind update, the oracle by freezing nodes in ascending order: tests/test_eikonal3_host.py shows
the two agree to 2e-14 of a cell's travel time on the CPU), so only rounding separates them; the roots are well conditioned where they are accepted
(discriminants >= s^2).  Grids are a few thousand nodes: one tile, no side a multiple of the tile, a side shorter than a tile, a side of two nodes.
Measured on an MI355X over the 60 maps of the first test: at most 2.2e-11 of the smallest cell travel time (2.2e-12 of the largest), at the 10 : 1 interface.

Sampler: the kernel takes its sums in the restatement's order, so only fused multiply-adds separate the two; the bound asked is 1e-12 relative, element by
element, bitwise on nodes, NaN exactly where the restatement has NaN.  Measured: at most 8.0e-16.

This file also holds the entries' STREAM CASES (``STREAM_CASES``): ``qdas_eikonal3`` and ``qdas_eikonal3_tables`` take their stream in the descriptor's
``queue`` field, because the census of ``void *stream`` parameters (tests/test_streams_host.py) is a pinned list."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from qups_amd import ChannelData, Scan, Sequence, Transducer, UltrasoundSystem, _lib, msfm3d
from qups_amd import eikonal as E
from tests import eikonal3_ref as R3
from tests import guards as GD
from tests import streams as ST

pytestmark = pytest.mark.gpu

DP = 0.25e-3
FILL_MS = 16                                  # tests/test_gpu_streams.py's: ten times the largest host time of a warm wrapper call
STREAM_CASES = ("test_stream_tables_behind_a_delayed_producer_return_early", "test_stream_solver_behind_a_delayed_producer_waits_for_its_stream")
BLOCKS = {"eikonal3": "qups_amd/csrc/eikonal3.hip:qdas_eikonal3 -- the host reads the list lengths back after every chunk of passes and ends the iteration "
                      "(include/qdas.h: qdas_eikonal3 WAITS for the stream)"}
GRIDS = [(8, 8, 8), (19, 13, 10), (17, 5, 9), (24, 16, 2)]
SPEEDS = ["homogeneous", "layers_ball", "smooth_random"]
IDS = lambda s: "x".join(str(v) for v in s) if isinstance(s, tuple) else str(s)


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _speed(kind, shape):
    c = {"homogeneous": lambda: np.full(shape, 1540.0), "layers_ball": lambda: R3.layers_ball(*shape),
         "smooth_random": lambda: R3.smooth_random(*shape, seed=sum(shape))}[kind]()
    c.setflags(write=False)
    return c


def _sets(shape):
    """five source sets, 1-based: a grid corner; a point on tile faces (node index 7 along dimension 1, 8 along dimension 2, where the grid has them);
    the tile corner (8, 8, 8) (clipped to the grid); three points in one set; fractional coordinates that floor"""
    C1, C2, C3 = shape
    return [np.array([[1.0], [1.0], [1.0]]),
            np.array([[min(8.0, C1)], [min(9.0, C2)], [(C3 + 1) // 2]]),
            np.array([[min(9.0, C1)], [min(9.0, C2)], [min(9.0, C3)]]),
            np.array([[1.0, C1, 0.5 * C1 + 0.6], [C2, 1.0, 0.5 * C2 + 0.7], [1.0, C3, 0.5 * C3 + 0.8]]),
            np.array([[0.7 * C1 + 0.99], [0.2 * C2 + 1.01], [0.45 * C3 + 0.9]])]


@functools.lru_cache(maxsize=None)
def _oracle(kind, shape):
    """the five maps of ``_sets(shape)``, computed once per module"""
    maps = tuple(R3.fmm3(_speed(kind, shape), DP, s) for s in _sets(shape))
    for m in maps:
        m.setflags(write=False)
    return maps


@functools.lru_cache(maxsize=None)
def _device(kind, shape):
    """the same five maps from ONE call (K = 5 sets share the launches), with passes and visits"""
    T = E.eikonal3(_speed(kind, shape), DP, _sets(shape))
    torch.cuda.synchronize()
    return T, E.eikonal3.last_passes, E.eikonal3.last_visits


# ---------------------------------------------------------------------------------------------------------------- maps
@pytest.mark.parametrize("kind", SPEEDS)
@pytest.mark.parametrize("shape", GRIDS, ids=IDS)
def test_maps_against_the_heap_oracle(shape, kind):
    c = _speed(kind, shape)
    T, passes, visits = _device(kind, shape)
    ref = _oracle(kind, shape)
    assert tuple(T.shape) == shape + (5,) and T.dtype == torch.float64
    bound = 1e-9 * DP / c.max()
    for k, r in enumerate(ref):
        t = _np(T[..., k])
        err = np.abs(t - r).max()
        print(f"{shape} {kind} set {k}: max |T - ref| = {err / (DP / c.max()):.3e} of the smallest cell time ({err / (DP / c.min()):.3e} of the largest)")
        assert np.isfinite(t).all() and err <= bound, (k, err, bound)
    tiles = int(np.prod([-(-n // 8) for n in shape]))
    print(f"{shape} {kind}: {passes} passes (cap {E.pass_cap3(*shape)}), {visits} tile visits = {visits / (5 * tiles * passes):.2f} of sets x tiles x passes")
    assert 0 < passes <= E.pass_cap3(*shape) and 5 <= visits <= 5 * tiles * passes


def test_one_set_per_call_equals_the_shared_launches_bit_for_bit():
    shape, kind = (19, 13, 10), "layers_ball"
    T, _, _ = _device(kind, shape)
    for k in (1, 3):
        one = E.eikonal3(_speed(kind, shape), DP, [_sets(shape)[k]])
        assert ST.same_bits(one[..., 0].contiguous(), T[..., k].contiguous())


def test_msfm3d_contract():
    """speed in cells per second, 1-based floored points, several points -> one map"""
    shape = (17, 5, 9)
    F = _speed("smooth_random", shape) / DP
    sp = _sets(shape)[3]
    T = _np(msfm3d(F, sp))
    assert T.shape == shape and T[0, 4, 0] == 0 and T[16, 0, 8] == 0 and T[8, 2, 4] == 0
    assert np.abs(T - _oracle("smooth_random", shape)[3]).max() <= 1e-9 / F.max()


# ---------------------------------------------------------------------------------------------------------------- cap and bases
def _direct(shape, c, src, base=1, max_passes=0, work_extra=0):
    """qdas_eikonal3 into tensors the test owns: ``(rc, T, passes, work)``; T starts as zeros"""
    C1, C2, C3 = shape
    cc = torch.from_numpy(np.ascontiguousarray(np.asarray(c, float).transpose(2, 1, 0))).cuda()
    src = np.ascontiguousarray(np.asarray(src, float).reshape(3, -1).T)
    T = torch.zeros((src.shape[0], C3, C2, C1), dtype=torch.float64, device="cuda")
    d = _lib.Eikonal3Desc()
    d.C1, d.C2, d.C3, d.K, d.npts, d.dp, d.base, d.max_passes, d.device = C1, C2, C3, src.shape[0], src.shape[0], DP, base, max_passes, -1
    d.queue = torch.cuda.current_stream().cuda_stream
    n, p = C.c_uint64(), C.c_uint32()
    assert _lib.lib().qdas_eikonal3_work_bytes(C.byref(d), C.byref(n)) == 0
    work = torch.full((n.value + work_extra,), 0xFF, dtype=torch.uint8, device="cuda")
    rc = _lib.lib().qdas_eikonal3(C.byref(d), C.c_void_p(cc.data_ptr()), C.c_void_p(src.ctypes.data), C.c_void_p(T.data_ptr()), C.c_void_p(work.data_ptr()),
                                  n.value, C.byref(p))
    torch.cuda.synchronize()
    return rc, T.permute(3, 2, 1, 0), p.value, work


def test_the_pass_cap_is_an_error_and_no_map():
    shape = (19, 13, 10)
    c = _speed("homogeneous", shape)
    with pytest.raises(_lib.QdasError) as ei:
        E.eikonal3(c, DP, [[1.0], [1.0], [1.0]], max_passes=1)
    assert ei.value.code == _lib.QDAS_ENOCONV and "no fixed point within 1 passes" in ei.value.message and E.eikonal3.last_passes == 1
    rc, T, passes, _ = _direct(shape, c, [[1.0], [1.0], [1.0]], max_passes=1)
    assert rc == _lib.QDAS_ENOCONV and passes == 1 and bool(torch.isnan(T).all())       # no unconverged map comes back
    rc, T, passes, _ = _direct(shape, c, [[1.0], [1.0], [1.0]])                          # the default cap: converges, and the library is as usable as before
    assert rc == 0 and 1 < passes <= E.pass_cap3(*shape) and bool(torch.isfinite(T).all())
    rc, T, passes, _ = _direct((8, 8, 8), _speed("homogeneous", (8, 8, 8)), [[3.0], [3.0], [3.0]], max_passes=1)
    assert rc == 0 and passes == 1 and bool(torch.isfinite(T).all())                     # one tile: 21 applications carry the front across, one pass


def test_base_0_is_base_1_shifted():
    shape = (17, 5, 9)
    c = _speed("smooth_random", shape)
    src = np.concatenate(_sets(shape)[:3] + [_sets(shape)[4]], axis=1)
    rc1, T1, _, _ = _direct(shape, c, src, base=1)
    rc0, T0, _, _ = _direct(shape, c, src - 1.0, base=0)
    assert rc0 == rc1 == 0 and ST.same_bits(T0.contiguous(), T1.contiguous())
    Pi = np.stack([np.random.default_rng(3).uniform(1, n, 40) for n in shape])
    assert ST.same_bits(E.eikonal3_tables(T1, Pi, base=1).contiguous(), E.eikonal3_tables(T1, Pi - 1.0, base=0).contiguous())


# ---------------------------------------------------------------------------------------------------------------- work space and guards
@pytest.mark.parametrize("shape,kind", [((19, 13, 10), "layers_ball"), ((24, 16, 2), "smooth_random")], ids=IDS)
def test_guarded_poisoned_maps_and_work_space(shape, kind, monkeypatch):
    """T and the work space come from torch.empty: inside the guard both lie between 64 KiB bands of 0xFF and start out as 0xFF themselves.  The bands stay
    intact, every node of every map is written, and the poisoned work space gives the maps of the plain call bit for bit"""
    T0, _, _ = _device(kind, shape)
    with GD.guard_outputs(monkeypatch) as g:
        T = E.eikonal3(_speed(kind, shape), DP, _sets(shape))
        assert len(g.bufs) == 2 and g.bufs[1].inner.dtype == torch.uint8            # the maps and the work space
        assert g.check(T) == 1
    assert ST.same_bits(T.contiguous(), T0.contiguous())


def test_work_space_followed_by_a_guard_band():
    """the library is told the exact size it asked for; the 64 KiB behind it stay 0xFF"""
    shape = (19, 13, 10)
    rc, T, _, work = _direct(shape, _speed("layers_ball", shape), np.concatenate(_sets(shape), axis=1)[:, :3], work_extra=GD.G)
    assert rc == 0 and bool((work[-GD.G:] == 0xFF).all())
    assert ST.same_bits(T[..., 1].contiguous(), _device("layers_ball", shape)[0][..., 1].contiguous())


def test_guarded_poisoned_tables(monkeypatch):
    shape = (19, 13, 10)
    T, _, _ = _device("smooth_random", shape)
    Pi = _pixels(shape, np.random.default_rng(5))
    ref = E.eikonal3_tables(T, Pi)
    with GD.guard_outputs(monkeypatch) as g:
        tau = E.eikonal3_tables(T, Pi)
        assert len(g.bufs) == 1 and g.check(tau) == 1                                # every element written (NaN outside is a written value), no byte beyond
    assert ST.same_bits(tau.contiguous(), ref.contiguous()) and bool(torch.isnan(tau).any())


# ---------------------------------------------------------------------------------------------------------------- sampler
def _pixels(shape, rng):
    """1-based coordinates 3 x I: every node; points in the outermost cells of every side; random interior points; points outside and NaN"""
    g = np.meshgrid(*(np.arange(n) + 1.0 for n in shape), indexing="ij")
    nodes = np.stack([x.ravel() for x in g])
    inner = np.stack([rng.uniform(1, n, 300) for n in shape])
    border = np.stack([rng.uniform(1, n, 240) for n in shape])
    for d, n in enumerate(shape):                                       # 40 points in the first and 40 in the last cell of each dimension
        border[d, 80 * d:80 * d + 40] = rng.uniform(1, min(2, n), 40)
        border[d, 80 * d + 40:80 * d + 80] = rng.uniform(max(n - 1, 1), n, 40)
    out = np.stack([rng.uniform(1, n, 12) for n in shape])
    for d, n in enumerate(shape):
        out[d, 4 * d], out[d, 4 * d + 1], out[d, 4 * d + 2] = 1 - 1e-9, n + 1e-9, np.nan
        out[d, 4 * d + 3] = -3.0
    return np.concatenate([nodes, inner, border, out], axis=1)


@pytest.mark.parametrize("shape", [(9, 7, 6), (2, 7, 3), (3, 2, 5), (5, 3, 1), (1, 1, 4)], ids=IDS)
def test_sampler_against_the_restatement(shape):
    rng = np.random.default_rng(sum(shape))
    maps = rng.uniform(1.0, 2.0, shape + (3,))
    Pi = _pixels(shape, rng)
    tau = _np(E.eikonal3_tables(torch.from_numpy(maps).cuda(), Pi))
    assert tau.shape == (Pi.shape[1], 3)
    nn = int(np.prod(shape))
    for k in range(3):
        ref = R3.sample3(maps[..., k], Pi)
        assert np.array_equal(np.isnan(tau[:, k]), np.isnan(ref)) and np.isnan(ref[-12:]).all() and not np.isnan(ref[:-12]).any()
        assert np.array_equal(tau[:nn, k], maps[..., k].ravel())                     # on a node: the node's value bit for bit
        ok = ~np.isnan(ref)
        rel = np.abs(tau[ok, k] - ref[ok]) / np.abs(ref[ok])
        print(f"{shape} map {k}: max relative deviation {rel.max():.3e}")
        assert np.abs(ref[ok]).min() > 0 and rel.max() <= 1e-12


# ---------------------------------------------------------------------------------------------------------------- streams
def test_stream_tables_behind_a_delayed_producer_return_early():
    """maps and pixel coordinates are all-0xFF twins that receive the true data on a non-blocking side stream behind FILL_MS of fills; the call, issued at
    once on that stream, and a clone taken directly behind it give the serial result bit for bit, and the wrapper returns while the filler is still running"""
    shape = (19, 13, 10)
    T, _, _ = _device("layers_ball", shape)
    Pi = torch.from_numpy(_pixels(shape, np.random.default_rng(6))).cuda()
    ref = E.eikonal3_tables(T, Pi).contiguous()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                                        # warm: allocator blocks of this stream, code objects
        E.eikonal3_tables(T, Pi)
    torch.cuda.synchronize()
    (tau,), (clone,), early = ST.run_delayed(E.eikonal3_tables, [T, Pi], side, FILL_MS)
    assert ST.same_bits(tau.contiguous(), ref) and ST.same_bits(clone.contiguous(), ref)
    assert early, "eikonal3_tables did not return before the queued work had run: it waits for the stream (or for the device), and is not in BLOCKS"


def test_stream_solver_behind_a_delayed_producer_waits_for_its_stream():
    """the speed volume is a poisoned twin filled behind the filler on a side stream: the solver, which runs on that stream, gives the serial maps bit for
    bit -- and has waited for the stream when it returns, as BLOCKS says (the table must stay true)"""
    shape, kind = (19, 13, 10), "layers_ball"
    T0, _, _ = _device(kind, shape)
    c = torch.from_numpy(np.ascontiguousarray(_speed(kind, shape))).cuda()
    fn = lambda ct: E.eikonal3(ct, DP, _sets(shape))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        fn(c)
    torch.cuda.synchronize()
    (T,), (clone,), early = ST.run_delayed(fn, [c], side, FILL_MS)
    assert ST.same_bits(T.contiguous(), T0.contiguous()) and ST.same_bits(clone.contiguous(), T0.contiguous())
    assert not early, f"BLOCKS lists 'eikonal3' ({BLOCKS['eikonal3']}) but the wrapper returned while the filler was still running"


# ---------------------------------------------------------------------------------------------------------------- end to end
C0, FC = 1500.0, 5e6
CGRD_X, CGRD_Z = np.arange(11) * 0.15e-3 - 0.75e-3, np.arange(33) * 0.15e-3          # 33 x 11 x 11 nodes; the elements lie on nodes of the plane z = 0


def _system(scan=None):
    xdc = Transducer.matrix(3, 0.3e-3, FC)
    scan = scan or Scan.cartesian(np.linspace(-0.6e-3, 0.6e-3, 9) + 0.01e-3, np.linspace(0.2e-3, 4.6e-3, 33), np.linspace(-0.55e-3, 0.55e-3, 9))
    return UltrasoundSystem(xdc, Sequence("FSA", c0=C0), scan, fs=8 * FC), Scan.cartesian(CGRD_X, CGRD_Z, CGRD_X)


def _cvolume():
    return 1400.0 + 0.2 * (R3.smooth_random(33, 11, 11, seed=8) - 1000.0)               # 1400 .. 1600 m/s


@functools.lru_cache(maxsize=None)
def _oracle_maps(homogeneous=False):
    """the nine elements' maps on the 33 x 11 x 11 grid by the heap oracle, computed once per module"""
    us, cgrd = _system()
    og, dp, dims, axes, size = E.scan_grid3(cgrd)
    g = E.grid_coordinates(us.rx.positions(), og, dp, axes)
    c = np.full(size, C0) if homogeneous else _cvolume()
    return tuple(R3.fmm3(c, dp, g[:, n:n + 1]) for n in range(g.shape[1]))


def _oracle_tables(us, cgrd, homogeneous=False):
    og, dp, dims, axes, size = E.scan_grid3(cgrd)
    Pi = E.grid_coordinates(np.asarray(us.scan.positions()).reshape(3, -1, order="F"), og, dp, axes)
    return np.stack([R3.sample3(m, Pi).reshape(us.scan.size, order="F") for m in _oracle_maps(homogeneous)], -1)


@functools.lru_cache(maxsize=None)
def _greens_data():
    us, _ = _system()
    t = np.arange(-2.0 / FC, 2.0 / FC, 1 / (32 * FC))
    wv = np.exp(-(t * FC * 1.2) ** 2) * np.exp(2j * np.pi * FC * t)
    chd = us.greens(np.array([[0.1e-3], [-0.15e-3], [2.5e-3]]), [1.0], wv, t[0], 32 * FC, R0=C0 / FC, focus=False)
    torch.cuda.synchronize()
    return chd


@pytest.mark.parametrize("keep", ["sum", "rx"])
def test_bfEikonal_volume_against_bfDASLUT_of_the_oracle_tables(keep):
    """a 3 x 3 matrix array, greens data of one scatterer, a 33 x 9 x 9-pixel volume inside a 33 x 11 x 11-node speed grid; the same consumer with the
    oracle's tables; tolerance: that of the das_lut-versus-oracle tests for complex64 data (1e-4), as tests/test_gpu_eikonal.py takes for the 2-D twin"""
    us, cgrd = _system()
    chd = _greens_data()
    assert chd.data.dtype == torch.complex64 and tuple(chd.data.shape[1:3]) == (9, 9)
    kw = dict(keep_rx=keep == "rx")
    b, tau_rx, tau_tx = us.bfEikonal(chd, _cvolume(), cgrd, return_delays=True, **kw)
    assert tuple(tau_rx.shape) == (33, 9, 9, 9) and tuple(tau_tx.shape) == (33, 9, 9, 1, 9)
    assert tau_tx.data_ptr() == tau_rx.data_ptr()                             # tx is rx: the transmit tables are the receive tables
    ref_rx = _oracle_tables(us, cgrd)
    assert not np.isnan(ref_rx).any()
    err_t = np.abs(_np(tau_rx) - ref_rx).max()
    print(f"tables: max err {err_t / (0.15e-3 / 1600.0):.3e} cell")
    assert err_t <= 1e-9 * 0.15e-3 / 1600.0 + 1e-12 * np.abs(ref_rx).max()
    ref = _np(us.bfDASLUT(chd, ref_rx, ref_rx, **kw))
    b = _np(b)
    err = np.abs(b - ref).max() / np.abs(ref).max()
    print(f"volume image, keep={keep}: rel err {err:.3e}")
    assert b.shape == ref.shape and np.abs(ref).max() > 0 and err <= 1e-4
    if keep == "sum":                                                          # the image peaks at the scatterer's pixel neighbourhood
        iz, ix, iy = np.unravel_index(np.argmax(np.abs(b).reshape(us.scan.size)), us.scan.size)
        P = us.scan.positions()[:, iz, ix, iy]
        assert np.all(np.abs(P - [0.1e-3, -0.15e-3, 2.5e-3]) <= [0.3e-3, 0.3e-3, 0.3e-3]), P


def test_delay_only_shapes_and_tables_on_the_grid_itself_are_the_maps():
    """scan == cgrd: table n IS map n at every pixel"""
    _, cgrd = _system()
    us, _ = _system(cgrd)
    c = _cvolume()
    b, tau_rx, tau_tx = us.bfEikonal(None, c, delay_only=True, keep_tx=True)
    assert tuple(b.shape) == (33, 11, 11, 1, 9, 0)
    assert tuple(tau_rx.shape) == (33, 11, 11, 9) and tuple(tau_tx.shape) == (33, 11, 11, 1, 9)
    og, dp, dims, axes, size = E.scan_grid3(cgrd)
    Tg = _np(E.eikonal3(c, dp, E.grid_coordinates(us.rx.positions(), og, dp, axes)))
    a = _np(tau_rx)
    assert np.all(np.abs(a - Tg) <= 1e-12 * np.abs(Tg))
    assert np.abs(a - np.stack(_oracle_maps(), -1)).max() <= 1e-9 * dp / c.max()


def test_pixels_outside_the_volume_are_nan_in_the_table_and_exactly_zero_in_the_image():
    big = Scan.cartesian(np.linspace(-1.2e-3, 1.2e-3, 9), np.linspace(0.2e-3, 5.6e-3, 33), np.linspace(-0.6e-3, 0.9e-3, 9))
    us, cgrd = _system(big)
    chd = _greens_data()
    b, tau_rx, tau_tx = us.bfEikonal(chd, C0, cgrd, return_delays=True)
    out = np.isnan(_np(tau_rx)).all(-1)
    assert out.any() and not out.all()
    assert np.array_equal(np.isnan(_np(tau_rx)).any(-1), out)                 # a pixel is outside for every element or for none
    img = _np(b).reshape(us.scan.size)
    assert np.all(img[out] == 0) and np.all(np.isfinite(img)) and np.abs(img[~out]).max() > 0
    ref_rx = _oracle_tables(us, cgrd, homogeneous=True)
    assert np.array_equal(np.isnan(ref_rx).all(-1), out)
    ref = _np(us.bfDASLUT(chd, ref_rx, ref_rx)).reshape(us.scan.size)
    assert np.abs(img - ref).max() / np.abs(ref).max() <= 1e-4


def test_sources_are_solved_in_blocks_under_a_map_budget():
    shape = (17, 5, 9)
    c = _speed("layers_ball", shape)
    src = np.concatenate([s[:, :1] for s in _sets(shape)] * 2, axis=1)[:, :7]
    Pi = _pixels(shape, np.random.default_rng(2))
    Isz = (Pi.shape[1], 1, 1)
    full = E.travel_time_tables3(c, DP, src, Pi, Isz)
    blocked = E.travel_time_tables3(c, DP, src, Pi, Isz, budget=2 * int(np.prod(shape)) * 8)     # two maps at a time
    assert tuple(full.shape) == Isz + (7,) and ST.same_bits(full.contiguous(), blocked.contiguous())
