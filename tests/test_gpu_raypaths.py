"""qdas_raypaths_weights / qdas_raypaths_integrate and their Python layer (qups_amd/raypaths.py) on the device, against the float64 restatement
tests/raypaths_ref.py and against the closed forms the contract implies (Liang-Barsky clipped length, exact integral of a linear field).

Grids: the smallest on which the walk can go wrong -- 2 x 2, the reference's 11 x 9 (and 9 x 11 for its swapped cases), a non-uniform 33 x 41 in metres with end
points up to a quarter of the span outside, 2 x 65 and 65 x 2.  Rays: tests/raypaths_ref.py ``rays`` (random, vertical, horizontal, on grid lines including the
last row / column, node to node, border, corners, misses, zero length, NaN / Inf) plus the reference's 32 sign / swap cases.

TOLERANCES.  Measured on an MI355X over every case of this file, max |dev - ref| / max |ref|; for float32 the restatement gets the float32-rounded grid and
points, so the figure is the kernel's error and not that of the inputs:
                 dense weights            integrals (length, linear field, constant map, the call's own triplets, delay tables)
    float64      8.9e-15 -> 4e-14         1.8e-15 -> 8e-15
    float32      4.3e-6  -> 2e-5          6.4e-7  -> 3e-6
Each bound is 4 x the measured value rounded up to one digit (the margin covers FMA contraction differences between compilers and boxes; the kernel forms its
crossings without the sort, so identical rounding with the restatement is not expected).  The largest figures come from the 33 x 41 millimetre grid (weights:
a crossing parameter carries eps x the number of cells of its axis relative to a cell) and from the 65-cell strips (integrals: 65 sums in sequence in the
data's precision, eps sqrt(65) = 5e-7 in float32); the same walk compiled for the host (tests/test_raypaths_host.py) gives 7.2e-15 and 3.4e-6 for the
weights.  A figure an order of magnitude above these means a segment in the wrong cell, not rounding.

This file also holds the entries' STREAM CASE (``STREAM_CASES``): both take their stream in the descriptor's ``queue`` field, because the census of ``void
*stream`` parameters (tests/test_streams_host.py) is a pinned list."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from qups_amd import DasError, _lib
from qups_amd import raypaths as RP
from qups_amd.interpd import das_lut
from tests import guards as GD
from tests import raypaths_ref as R
from tests import streams as ST

pytestmark = pytest.mark.gpu

MEASURED = {("w", torch.float64): 8.9e-15, ("i", torch.float64): 1.8e-15, ("w", torch.float32): 4.3e-6, ("i", torch.float32): 6.4e-7}      # MI355X, every case below
TOL = {("w", torch.float64): 4e-14, ("i", torch.float64): 8e-15, ("w", torch.float32): 2e-5, ("i", torch.float32): 3e-6}                      # 4 x, rounded up to one digit
STREAM_CASES = ("test_stream_delayed_producer_on_a_side_stream",)
FILL_MS = 60
SENTINEL = 0x5A5A5A5A
DTYPES = [torch.float64, torch.float32]
GRIDS = ["2x2", "11x9", "9x11", "33x41", "2x65", "65x2"]
NP = {torch.float64: np.float64, torch.float32: np.float32}


def _rnd(a, dtype):
    """the values the device sees, as float64"""
    return np.asarray(a, NP[dtype]).astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(name, dtype):
    """grid, rays, the restatement's dense weights (J x X x Z), the clipped lengths and the integrals of a linear field -- computed once, never modified"""
    if name == "9x11":
        cs = R.sign_swap_cases()[16:]
        xg, zg = cs[0][0], cs[0][1]
        pa, pb = np.stack([c[2] for c in cs], 1), np.stack([c[3] for c in cs], 1)
    else:
        xg, zg = R.grids()[name]
        pa, pb = R.rays(xg, zg)
        if name == "11x9":
            cs = R.sign_swap_cases()[:16]
            pa = np.concatenate([pa, np.stack([c[2] for c in cs], 1)], 1)
            pb = np.concatenate([pb, np.stack([c[3] for c in cs], 1)], 1)
    xg, zg, pa, pb = (_rnd(v, dtype) for v in (xg, zg, pa, pb))
    J = pa.shape[1]
    W = R.dense_many(xg, zg, pa, pb)
    L = np.array([R.clipped_length(xg, zg, pa[:, j], pb[:, j]) for j in range(J)])
    lin = (0.3, 1.7 / np.ptp(xg), -0.9 / np.ptp(zg))
    Il = np.array([R.linear_integral(xg, zg, pa[:, j], pb[:, j], *lin) for j in range(J)])
    for v in (xg, zg, pa, pb, W, L, Il):
        v.setflags(write=False)
    return dict(xg=xg, zg=zg, pa=pa, pb=pb, W=W, L=L, lin=lin, Il=Il, J=J)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def desc(xg, zg, pa, pb, J, dtype, sa=1, sb=1, F=0, xstride=1, zstride=1, stream=None):
    d = _lib.RaypathsDesc()
    d.X, d.Z, d.J, d.F = xg.numel(), zg.numel(), J, F
    d.xstride, d.zstride, d.pa_stride, d.pb_stride = xstride, zstride, sa, sb
    d.dtype, d.device = (_lib.QDAS_F32 if dtype == torch.float32 else _lib.QDAS_F64), -1
    d.xg, d.zg, d.pa, d.pb = (C.c_void_p(t.data_ptr()) for t in (xg, zg, pa, pb))
    d.queue = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    return d


def raw_weights(c, dtype, pa=None, pb=None, J=None, sa=1, sb=1):
    """the C entry on guarded, poisoned outputs: ``(w, ix, iz)`` as numpy ``J x K x 4``.  Checks the guard bands of all three, that every real of ``w`` was
    written (0xFF poison) and that no index still holds the sentinel (-1 is a legal index value, so the indices get a poison of their own)."""
    xg, zg = dev(c["xg"], dtype), dev(c["zg"], dtype)
    pa = c["pa"] if pa is None else pa
    pb = c["pb"] if pb is None else pb
    J = max(pa.shape[1], pb.shape[1]) if J is None else J
    a, b = dev(pa.T, dtype), dev(pb.T, dtype)                                 # J x 2: (x, z) pairs
    K = int(_lib.lib().qdas_raypaths_slots(xg.numel(), zg.numel()))
    assert K == xg.numel() + zg.numel() + 1
    g = GD.Guard()
    w = g.empty((J, K, 4), dtype, "cuda")
    ix, iz = g.empty((J, K, 4), torch.int32, "cuda"), g.empty((J, K, 4), torch.int32, "cuda")
    ix.fill_(SENTINEL)
    iz.fill_(SENTINEL)
    d = desc(xg, zg, a, b, J, dtype, sa, sb)
    _lib.check(_lib.lib().qdas_raypaths_weights(C.byref(d), C.c_void_p(w.data_ptr()), C.c_void_p(ix.data_ptr()), C.c_void_p(iz.data_ptr())))
    assert g.check(w) == 1
    w, ix, iz = w.cpu().numpy(), ix.cpu().numpy(), iz.cpu().numpy()
    assert not (ix == SENTINEL).any() and not (iz == SENTINEL).any(), "an index slot was never written"
    return w, ix, iz


def check_triplets(w, ix, iz, X, Z):
    """indices in range or -1 (both or neither), the corner pattern of a slot, an empty slot weighs nothing, no weight negative or non-finite"""
    empty = ix < 0
    assert ((ix == -1) == (iz == -1)).all() and (ix >= -1).all() and (iz >= -1).all() and (ix < X).all() and (iz < Z).all()
    assert (empty.all(axis=2) | (~empty).all(axis=2)).all()
    full = ~empty[:, :, 0]
    assert (ix[full][:, [1, 3]] == ix[full][:, [0, 2]] + 1).all() and (iz[full][:, [2, 3]] == iz[full][:, [0, 1]] + 1).all()
    assert (ix[full][:, 0] == ix[full][:, 2]).all() and (iz[full][:, 0] == iz[full][:, 1]).all()
    assert (w[empty] == 0).all() and np.isfinite(w).all() and (w >= 0).all()


def dense_of(w, ix, iz, X, Z):
    J = w.shape[0]
    W = np.zeros((J, X, Z))
    v = ix >= 0
    j = np.broadcast_to(np.arange(J)[:, None, None], w.shape)
    np.add.at(W, (j[v], ix[v], iz[v]), w[v].astype(np.float64))
    return W


def rel(a, b):
    return float(np.abs(np.asarray(a) - b).max() / np.abs(b).max())


# ---------------------------------------------------------------------------------------------------------------- the weights entry
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", GRIDS)
def test_weights_against_the_restatement_and_the_closed_forms(name, dtype):
    c = case(name, dtype)
    X, Z = c["xg"].size, c["zg"].size
    w, ix, iz = raw_weights(c, dtype)
    check_triplets(w, ix, iz, X, Z)
    W = dense_of(w, ix, iz, X, Z)
    XX, ZZ = np.meshgrid(c["xg"], c["zg"], indexing="ij")
    fld = c["lin"][0] + c["lin"][1] * XX + c["lin"][2] * ZZ
    ew, el, ei = rel(W, c["W"]), rel(W.sum((1, 2)), c["L"]), rel((W * fld).sum((1, 2)), c["Il"])
    print(f"raypaths weights {name} {dtype}: J={c['J']} dense {ew:.3e} length {el:.3e} linear field {ei:.3e}")
    assert ew <= TOL["w", dtype] and el <= TOL["i", dtype] and ei <= TOL["i", dtype]
    dead = c["L"] == 0
    assert dead.any() or name == "9x11"
    assert (ix[dead] == -1).all() and (w[dead] == 0).all(), "a ray that misses the grid, has no length or a non-finite coordinate emitted a weight"
    assert (W[c["W"] == 0] <= TOL["w", dtype] * c["W"].max()).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_rays_along_grid_lines_weigh_only_that_line(dtype):
    """exactly: a crossing puts the point ON the grid value, so the neighbours' hats are 0 there -- in the last row and column too"""
    c = case("33x41", dtype)
    xg, zg = c["xg"], c["zg"]
    X, Z = xg.size, zg.size
    cols, rows = [0, 7, X - 1], [0, 20, Z - 1]
    pa = np.array([[xg[i], zg[0]] for i in cols] + [[xg[-1], zg[k]] for k in rows]).T
    pb = np.array([[xg[i], zg[-1]] for i in cols] + [[xg[0], zg[k]] for k in rows]).T
    W = dense_of(*raw_weights(c, dtype, pa, pb), X, Z)
    for n, i in enumerate(cols):
        off = np.delete(W[n], i, axis=0)
        assert (off == 0).all() and abs(W[n, i].sum() - (zg[-1] - zg[0])) <= TOL["i", dtype] * (zg[-1] - zg[0])
    for n, k in enumerate(rows):
        off = np.delete(W[3 + n], k, axis=1)
        assert (off == 0).all() and abs(W[3 + n, :, k].sum() - (xg[-1] - xg[0])) <= TOL["i", dtype] * (xg[-1] - xg[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_node_to_node_diagonals_on_a_square_grid(dtype):
    """the closed form of tests/test_raypaths_host.py ``diagonal_weights``: sqrt(2) d / 3 per crossed cell for the corners on the diagonal, / 6 for those off it"""
    from tests.test_raypaths_host import diagonal_weights
    d = 0.25
    g = d * np.arange(9.0)
    ends = ((1, 1, 6, 6), (7, 2, 3, 6), (0, 8, 8, 0), (8, 8, 0, 0))
    pa, pb = np.array([[g[e[0]], g[e[1]]] for e in ends]).T, np.array([[g[e[2]], g[e[3]]] for e in ends]).T
    w, ix, iz = raw_weights(dict(xg=g, zg=g), dtype, pa, pb)
    check_triplets(w, ix, iz, 9, 9)
    W = dense_of(w, ix, iz, 9, 9)
    for n, e in enumerate(ends):
        want = diagonal_weights(9, d, *e)
        assert np.abs(W[n] - want).max() <= TOL["w", dtype] * want.max() and (W[n][want == 0] == 0).all()


@pytest.mark.parametrize("J", [1, 63, 65, 257])
def test_ray_counts_around_the_wave_and_the_workgroup(J):
    dtype = torch.float64
    c = case("11x9", dtype)
    sel = np.arange(J) % c["J"]
    w, ix, iz = raw_weights(c, dtype, c["pa"][:, sel], c["pb"][:, sel])
    check_triplets(w, ix, iz, 11, 9)
    assert rel(dense_of(w, ix, iz, 11, 9), c["W"][sel]) <= TOL["w", dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_point_strides_of_zero_broadcast_one_point(dtype):
    c = case("33x41", dtype)
    J = c["J"]
    one = c["pa"][:, 12:13]
    ref = R.dense_many(c["xg"], c["zg"], one, c["pb"])
    for sa, sb, pa, pb in ((0, 1, one, c["pb"]), (1, 0, c["pb"], one)):
        w, ix, iz = raw_weights(c, dtype, pa, pb, J=J, sa=sa, sb=sb)
        e = rel(dense_of(w, ix, iz, 33, 41), ref)
        print(f"raypaths strides ({sa}, {sb}) {dtype}: dense {e:.3e}")
        assert e <= TOL["w", dtype]


# ---------------------------------------------------------------------------------------------------------------- the integrate entry
def maps_for(c, F, rng):
    """F maps as ``F x X x Z`` float64: the linear field, a constant, a random one"""
    XX, ZZ = np.meshgrid(c["xg"], c["zg"], indexing="ij")
    m = [c["lin"][0] + c["lin"][1] * XX + c["lin"][2] * ZZ, np.full(XX.shape, 0.65), rng.uniform(0.5, 1.5, XX.shape)]
    return np.stack(m[:F])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("ord", ["ZX", "XZ"])
@pytest.mark.parametrize("name,F", [("2x2", 1), ("11x9", 3), ("33x41", 3), ("33x41", 1), ("2x65", 1), ("65x2", 3)])
def test_integrate_against_its_own_triplets_and_the_closed_forms(name, F, ord, dtype, monkeypatch):
    c = case(name, dtype)
    X, Z = c["xg"].size, c["zg"].size
    m = _rnd(maps_for(c, F, np.random.default_rng(3)), dtype)                   # F x X x Z, the values the device sees
    maps = dev(m if ord == "XZ" else m.transpose(0, 2, 1), dtype)
    if F == 1:
        maps = maps[0]
    with GD.guard_outputs(monkeypatch) as g:
        y, ln = RP.ray_integrals(maps, c["xg"], c["zg"], dev(c["pa"], dtype), dev(c["pb"], dtype), ord=ord)
        assert g.check(y, ln) == 2
    assert tuple(y.shape) == ((F, c["J"]) if F > 1 else (c["J"],)) and tuple(ln.shape) == (c["J"],) and y.dtype == dtype
    y, ln = y.cpu().numpy().reshape(F, -1), ln.cpu().numpy()
    W = dense_of(*raw_weights(c, dtype), X, Z)
    own = np.einsum("jxz,fxz->fj", W, m)
    e_own, e_len, e_sum = rel(y, own), rel(ln, c["L"]), rel(ln, W.sum((1, 2)))
    e_lin = rel(y[0], c["Il"])
    e_const = rel(y[1], 0.65 * c["L"]) if F > 1 else 0.0
    print(f"raypaths integrate {name} F={F} {ord} {dtype}: own triplets {e_own:.3e} length {e_len:.3e} len-vs-weights {e_sum:.3e} linear {e_lin:.3e} constant {e_const:.3e}")
    assert max(e_own, e_len, e_sum, e_lin, e_const) <= TOL["i", dtype]
    dead = c["L"] == 0
    assert (y[:, dead] == 0).all() and (ln[dead] == 0).all()


def test_integrate_takes_a_strided_map_and_no_length():
    """a map that is a view of a larger array (its own strides travel in the descriptor), and ``len = NULL``"""
    dtype = torch.float64
    c = case("11x9", dtype)
    big = torch.from_numpy(np.random.default_rng(8).uniform(0.5, 1.5, (2 * 9, 3 * 11))).cuda()
    view = big[::2, 1::3]                                                        # Z x X
    assert not view.is_contiguous()
    y, _ = RP.ray_integrals(view, c["xg"], c["zg"], c["pa"], c["pb"])
    y2, _ = RP.ray_integrals(view.contiguous(), c["xg"], c["zg"], c["pa"], c["pb"])
    assert ST.same_bits(y, y2)
    xg, zg, a, b = dev(c["xg"], dtype), dev(c["zg"], dtype), dev(c["pa"].T, dtype), dev(c["pb"].T, dtype)
    m = view.contiguous()
    out = GD.guarded_empty((c["J"],), dtype, "cuda")
    d = desc(xg, zg, a, b, c["J"], dtype, F=1, xstride=1, zstride=11)
    _lib.check(_lib.lib().qdas_raypaths_integrate(C.byref(d), C.c_void_p(m.data_ptr()), C.c_void_p(out.data_ptr()), None))
    GD.check(out)
    assert ST.same_bits(out, y)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_two_runs_give_the_same_bits(dtype):
    c = case("33x41", dtype)
    a = raw_weights(c, dtype)
    b = raw_weights(c, dtype)
    assert all(np.array_equal(p.view(np.uint8), q.view(np.uint8)) for p, q in zip(a, b))
    maps = dev(maps_for(c, 3, np.random.default_rng(3)).transpose(0, 2, 1), dtype)
    r1 = RP.ray_integrals(maps, c["xg"], c["zg"], c["pa"], c["pb"])
    r2 = RP.ray_integrals(maps, c["xg"], c["zg"], c["pa"], c["pb"])
    assert ST.same_bits(r1[0], r2[0]) and ST.same_bits(r1[1], r2[1])


def test_stream_delayed_producer_on_a_side_stream():
    """grid, points and map are all-0xFF twins that receive the true data on a non-blocking side stream behind FILL_MS of fills; both entries, issued at once
    on that stream, and clones taken directly behind them give the serial result bit for bit, and the wrappers return while the filler is still running"""
    dtype = torch.float32
    c = case("33x41", dtype)
    xg, zg, a, b = dev(c["xg"], dtype), dev(c["zg"], dtype), dev(c["pa"].T, dtype), dev(c["pb"].T, dtype)
    maps = dev(maps_for(c, 3, np.random.default_rng(3)).transpose(0, 2, 1), dtype)
    J = c["J"]

    def fn(xg, zg, a, b, maps):
        w, ix, iz = RP._weights(xg, zg, a, b, J, 1, 1, dtype, xg.device)
        y = torch.empty((3, J), dtype=dtype, device="cuda")
        ln = torch.empty((J,), dtype=dtype, device="cuda")
        RP._integrate_into(y, ln, maps, xg, zg, a, b, J, 1, 1, dtype, xg.device, 1, 33)
        return w, ix, iz, y, ln

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                                            # warm: allocator blocks of this stream, code objects
        fn(xg, zg, a, b, maps)
    torch.cuda.synchronize()
    want = fn(xg, zg, a, b, maps)
    torch.cuda.synchronize()
    got, clones, early = ST.run_delayed(fn, [xg, zg, a, b, maps], side, FILL_MS)
    for g, cl, wt in zip(got, clones, want):
        assert ST.same_bits(g, wt) and ST.same_bits(cl, wt)
    assert early, "the wrappers did not return before the queued work had run: they wait for the stream (or for the device)"
    assert np.isfinite(want[3].cpu().numpy()).all()


# ---------------------------------------------------------------------------------------------------------------- the Python layer
def test_wbilerpg_shapes_and_the_documented_example():
    """the example of the reference's wbilerp.m: grid -5:5 x -5:5, (-4, 1) -> (3, -2); end points of shape 2 x 3"""
    x = y = np.arange(-5.0, 6.0)
    xa, ya, xb, yb = (np.full((2, 3), v) for v in (-4.0, 1.0, 3.0, -2.0))
    xa[1, 2], yb[0, 1] = 2.5, 4.25
    cxy, ixo, iyo = RP.wbilerpg(x, y, xa, ya, xb, yb)
    assert tuple(cxy.shape) == tuple(ixo.shape) == tuple(iyo.shape) == (4, 23, 2, 3) and ixo.dtype == torch.int32 and cxy.dtype == torch.float64
    for j, k in ((0, 0), (1, 2), (0, 1)):
        w, ix, iz = (t[:, :, j, k].permute(1, 0).unsqueeze(0).cpu().numpy() for t in (cxy, ixo, iyo))
        ref = R.dense(x, y, (xa[j, k], ya[j, k]), (xb[j, k], yb[j, k]))
        assert rel(dense_of(w, ix, iz, 11, 11)[0], ref) <= TOL["w", torch.float64]
    assert RP.wbilerpg(x.astype(np.float32), y.astype(np.float32), *(v.astype(np.float32) for v in (xa, ya, xb, yb)))[0].dtype == torch.float32
    assert RP.wbilerpg(x, y, xa, ya, xb, yb, r=[])[0].shape == cxy.shape
    with pytest.raises(NotImplementedError, match="r"):
        RP.wbilerpg(x, y, xa, ya, xb, yb, r=[0.5])


@pytest.mark.parametrize("ord", ["ZX", "XZ"])
def test_raypaths_dense_equals_the_documented_example(ord):
    """rayPaths.m's example: x = -5:5, z = -4:4, rays from (0, 0) to (-4, 1) and (3, -2)"""
    x, z = np.arange(-5.0, 6.0), np.arange(-4.0, 5.0)
    pj = np.array([[-4.0, 3.0], [1.0, -2.0]])
    w, d = RP.rayPaths(x, z, pj, np.array([0.0, 0.0]), ord=ord)
    assert w.is_sparse and w.is_coalesced() and tuple(w.shape) == (99 * 2, 1) and tuple(d.shape) == (2, 1)
    full = w.to_dense().cpu().numpy().reshape(2, 11, 9) if ord == "ZX" else w.to_dense().cpu().numpy().reshape(2, 9, 11).transpose(0, 2, 1)
    ref = R.dense_many(x, z, np.zeros((2, 1)), pj)
    assert rel(full, ref) <= TOL["w", torch.float64]
    assert np.allclose(d.cpu().numpy()[:, 0], np.hypot(pj[0], pj[1]), rtol=1e-15)
    assert abs(full[0].sum() - np.hypot(4, 1)) <= 1e-14 and abs(full[1].sum() - np.hypot(3, 2)) <= 1e-14


def test_raypaths_broadcasts_j_against_m_chunks_and_keeps_the_full_length():
    x, z = R.grids()["33x41"]
    rng = np.random.default_rng(4)
    J, M = 5, 3
    pj = np.stack((rng.uniform(x[0], x[-1], (J, 1)), rng.uniform(z[0], z[-1], (J, 1))))           # 2 x J x 1
    pa = np.stack((rng.uniform(x[0] - 5e-3, x[-1], (1, M)), np.full((1, M), z[0] - 2e-3)))          # 2 x 1 x M: outside the grid
    w, d = RP.rayPaths(x, z, pj, pa)
    w2, d2 = RP.rayPaths(x, z, pj, pa, bsize=2)
    I = x.size * z.size
    assert tuple(w.shape) == (I * J, M) and tuple(d.shape) == (J, M)
    assert torch.equal(w.to_dense(), w2.to_dense()) and torch.equal(d, d2)
    full = w.to_dense().cpu().numpy().reshape(J, x.size, z.size, M)
    dn = d.cpu().numpy()
    for j in range(J):
        for m in range(M):
            a, b = pa[:, 0, m], pj[:, j, 0]
            assert abs(dn[j, m] - np.hypot(*(a - b))) <= 4e-15 * dn[j, m]
            assert rel(full[j, :, :, m], R.dense(x, z, a, b)) <= TOL["w", torch.float64]
            assert full[j, :, :, m].sum() < dn[j, m]                                                  # clipped weights, full length
    with pytest.raises(NotImplementedError, match="xiaolin"):
        RP.rayPaths(x, z, pj, pa, method="xiaolin")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_global_average_c_homogeneous_layered_and_out_of_bounds(dtype):
    x, z = 1e-3 * np.linspace(-5, 5, 21), 1e-3 * np.linspace(0, 40, 81)
    tol = TOL["i", dtype]                          # c_avg = l / integral: the quotient of two quantities inside ``tol`` each, against a float64 reference on the
    c0 = torch.full((z.size, x.size), 1540.0, dtype=dtype, device="cuda")
    # unrounded grid (float32: another eps or two): 4 tol
    pb = np.array([[0.0, 2.2e-3, -5e-3, 5.1e-3, 0.0, 1e-3], [10e-3, 33.3e-3, 40e-3, 10e-3, 41e-3, -1e-3]])
    got = RP.globalAverageC(c0, x, z, np.array([0.0, 0.0]), pb).cpu().numpy()
    assert got.shape == (6,) and np.isnan(got[3:]).all(), "pb outside the scan bounds is NaN"
    assert np.abs(got[:3] / 1540.0 - 1).max() <= 4 * tol
    # layers: the speed is bilinear between the nodes, so along a grid column the integral of the slowness is the trapezoid sum of the node slownesses
    cz = np.where(z > 30e-3, 1400.0, np.where(z > 20e-3, 1600.0, 1500.0))
    cl = torch.from_numpy(np.repeat(cz[:, None], x.size, 1)).to("cuda", dtype)
    k = [8, 40, 41, 60, 61, 80]
    pbz = np.array([[x[10]] * len(k), z[k]])
    got = RP.globalAverageC(cl, x, z, np.array([x[10], z[0]]), pbz).cpu().numpy()
    s = 1 / _rnd(cz, dtype)
    trap = np.array([np.sum(0.5 * (s[1:kk + 1] + s[:kk]) * np.diff(z[:kk + 1])) for kk in k])
    want = (z[k] - z[0]) / trap
    print(f"globalAverageC layered {dtype}: {np.abs(got / want - 1).max():.3e}")
    assert np.abs(got / want - 1).max() <= 4 * tol
    # XZ order and the 2 x A extension
    pa2 = np.array([[0.0, x[3]], [0.0, z[5]]])
    g2 = RP.globalAverageC(cl.t().contiguous(), x, z, pa2, pbz, order="XZ").cpu().numpy()
    assert g2.shape == (len(k), 2) and np.abs(g2[:, 0] / RP.globalAverageC(cl, x, z, pa2[:, 0], pbz).cpu().numpy() - 1).max() <= 4 * tol
    assert np.isnan(RP.globalAverageC(cl, x, z, [x[10], z[0]], np.array([[x[10]], [z[0]]])).cpu().numpy()).all(), "a ray of no length: 0 / 0, then NaN"


def test_straight_ray_tables_of_a_homogeneous_map_feed_das_lut():
    """32 elements, 32 x 32 pixels: the tables ray_integrals gives for a homogeneous slowness map are the geometric delays, and das_lut makes the same image from
    either -- within that entry's own tolerances (tests/test_gpu_golden.py: 1e-9 double, 5e-4 single, cubic)"""
    rng = np.random.default_rng(6)
    N = M = 32
    c0, fs, T = 1540.0, 20e6, 1400
    xe = np.linspace(-9.3e-3, 9.3e-3, N)
    x, z = np.linspace(-10e-3, 10e-3, 41), np.linspace(0.0, 45e-3, 91)
    px, pz = np.meshgrid(np.linspace(-8e-3, 8e-3, 32), np.linspace(10e-3, 40e-3, 32), indexing="ij")
    pix = np.stack((px.reshape(-1), pz.reshape(-1)))                              # 2 x I
    slow = torch.full((z.size, x.size), 1 / c0, dtype=torch.float64, device="cuda")
    pixd = dev(pix, torch.float64)
    tau = torch.stack([RP.ray_integrals(slow, x, z, np.array([xe[n], 0.0]), pixd)[0] for n in range(N)], dim=1)      # I x N [s]
    geo = np.hypot(pix[0][:, None] - xe[None, :], pix[1][:, None]) / c0
    e = rel(tau.cpu().numpy(), geo)
    print(f"straight-ray table against the geometric delays: {e:.3e}")
    assert e <= TOL["i", torch.float64]
    data = torch.from_numpy((rng.standard_normal((T, N, M)) + 1j * rng.standard_normal((T, N, M))))
    for prec, tol in (("double", 1e-9), ("single", 5e-4)):
        a = das_lut(data, tau * fs, tau * fs, interp="cubic", prec=prec).cpu().numpy()
        b = das_lut(data, geo * fs, geo * fs, interp="cubic", prec=prec).cpu().numpy()
        assert np.abs(b).max() > 0 and rel(a, b) <= tol


def test_python_refusals_on_the_device():
    x, z = np.arange(4.0), np.arange(5.0)
    m = torch.zeros((5, 4), device="cuda")
    with pytest.raises(DasError, match="5 x 4"):
        RP.ray_integrals(m.t(), x, z, [0, 0], [1, 1])
    with pytest.raises(DasError, match="monotonic"):
        RP.ray_integrals(m, torch.tensor([0.0, 2.0, 1.0, 3.0], device="cuda"), z, [0, 0], [1, 1])
    with pytest.raises(DasError, match="float32 or float64"):
        RP.ray_integrals(m.half(), x, z, [0, 0], [1, 1])
    y, ln = RP.ray_integrals(m, x, z, np.zeros((2, 0)), np.zeros((2, 0)))
    assert tuple(y.shape) == (0,) and tuple(ln.shape) == (0,)
