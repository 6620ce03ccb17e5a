"""qdas_raypaths_backproject and its Python layer (qups_amd.ray_backproject, qups_amd.ray_sart) on the device, against the float64 restatement
tests/raypaths_ref.py (``einsum(dense_many, r)`` and its column sums), against the device's own forward operator (the adjoint identity) and against SART in
numpy on the restatement's matrix (tests/raysart_ref.py).

Grids: the five of raypaths_ref.grids() (and 9 x 11 for the reference's swapped sign cases) plus the smallest that sit on the edges of the kernel's 8 x 8
tiles and their one-line halo: 8 x 8 (one full tile), 9 x 9 (a second tile of one row and column), 17 x 7 (three tiles along x, a part of one along z); 2 x 2 is
among the five.  Rays: raypaths_ref.rays() -- random, vertical, horizontal, on grid lines including the last row / column, node to node, border, corners,
misses, zero length, NaN / Inf.

TOLERANCES.  Measured on an MI355X over every case of this file, max |dev - ref| / max |ref|; for float32 the restatement gets the float32-rounded grid,
points and residuals, so the figure is the kernel's error and not that of the inputs:
                 back-projection and column sums      SART, after 1 and 10 steps      adjoint identity, c
    float64      5.1e-15 -> 3e-14                     9.8e-16 -> 4e-15                0.072 -> 0.3
    float32      1.4e-6  -> 6e-6                      4.2e-7  -> 2e-6                 0.082 -> 0.4
The largest figures of the products come from the 33 x 41 millimetre grid (the same walk compiled for the host, tests/test_raybackproject_host.py, gives
7.3e-15 and 2.8e-6 there against rays of every kind at once).  Each bound is 4 x the measured value rounded up to one digit, under a cap that is not measured: 1e-12 and 1e-4
for the products (a figure above it is a segment in the wrong cell, not rounding), and for SART the same caps -- ten steps of a non-expansive iteration
(relax = 1) pass the products' errors on, they do not amplify them.  The adjoint identity's constant ``c`` in
``|<A s, r> - <s, A' r>| <= c eps <A |s|, |r|>`` is measured the same way under the cap 64: a random-sign sum of n terms errs by about eps sqrt(n) of its
largest partial sum, far below eps sum |terms|.

This file also holds the entry's STREAM CASE (``STREAM_CASES``): it takes its stream in the descriptor's ``queue`` field, because the census of ``void
*stream`` parameters (tests/test_streams_host.py) is a pinned list."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import qups_amd
from qups_amd import DasError, _lib
from qups_amd import raypaths as RP
from tests import guards as GD
from tests import raypaths_ref as R
from tests import raysart_ref as S
from tests import streams as ST

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
MEASURED = {("g", F64): 5.1e-15, ("g", F32): 1.4e-6, ("sart", F64): 9.8e-16, ("sart", F32): 4.2e-7, ("adj", F64): 0.072, ("adj", F32): 0.082}     # MI355X, every case below
TOL = {("g", F64): 3e-14, ("g", F32): 6e-6, ("sart", F64): 4e-15, ("sart", F32): 2e-6, ("adj", F64): 0.3, ("adj", F32): 0.4}                        # 4 x, rounded up to one digit
CAP = {("g", F64): 1e-12, ("g", F32): 1e-4, ("sart", F64): 1e-12, ("sart", F32): 1e-4, ("adj", F64): 64.0, ("adj", F32): 64.0}
STREAM_CASES = ("test_stream_delayed_producer_on_a_side_stream",)
FILL_MS = 60
DTYPES = [F64, F32]
GRIDS = ["2x2", "11x9", "9x11", "33x41", "2x65", "65x2", "8x8", "9x9", "17x7"]
NP = {F64: np.float64, F32: np.float32}
EPS = {F64: float(np.finfo(np.float64).eps), F32: float(np.finfo(np.float32).eps)}


def test_every_bound_is_four_times_its_measurement_under_its_cap():
    for k in TOL:
        assert 4 * MEASURED[k] <= TOL[k] <= CAP[k], k


def _rnd(a, dtype):
    """the values the device sees, as float64"""
    return np.asarray(a, NP[dtype]).astype(np.float64)


def grid_of(name):
    if name in R.grids():
        return R.grids()[name]
    X, Z = (int(v) for v in name.split("x"))
    rng = np.random.default_rng(100 * X + Z)
    return 1e-3 * np.cumsum(rng.uniform(0.5, 1.5, X)), 1e-3 * np.cumsum(rng.uniform(0.5, 1.5, Z))


@functools.lru_cache(maxsize=None)
def case(name, dtype):
    """grid, rays, three residual vectors, the restatement's dense weights (J x X x Z) and the clipped lengths -- computed once, never modified"""
    if name == "9x11":
        cs = R.sign_swap_cases()[16:]
        xg, zg = cs[0][0], cs[0][1]
        pa, pb = np.stack([c[2] for c in cs], 1), np.stack([c[3] for c in cs], 1)
    else:
        xg, zg = grid_of(name)
        pa, pb = R.rays(xg, zg)
        if name == "11x9":
            cs = R.sign_swap_cases()[:16]
            pa = np.concatenate([pa, np.stack([c[2] for c in cs], 1)], 1)
            pb = np.concatenate([pb, np.stack([c[3] for c in cs], 1)], 1)
    xg, zg, pa, pb = (_rnd(v, dtype) for v in (xg, zg, pa, pb))
    J = pa.shape[1]
    r = _rnd(np.random.default_rng(17).standard_normal((3, J)), dtype)
    W = R.dense_many(xg, zg, pa, pb)
    L = np.array([R.clipped_length(xg, zg, pa[:, j], pb[:, j]) for j in range(J)])
    for v in (xg, zg, pa, pb, r, W, L):
        v.setflags(write=False)
    return dict(xg=xg, zg=zg, pa=pa, pb=pb, r=r, W=W, L=L, J=J, X=xg.size, Z=zg.size)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def rel(a, b):
    return float(np.abs(np.asarray(a) - b).max() / np.abs(b).max())


def xz(t, ord):
    """a map (or a stack of maps) of the Python layer as numpy ``... x X x Z``"""
    a = t.cpu().numpy().astype(np.float64)
    return a if ord == "XZ" else np.swapaxes(a, -1, -2)


def desc(xg, zg, pa, pb, J, dtype, sa=1, sb=1, F=0, xstride=1, zstride=1, stream=None):
    d = _lib.RaypathsDesc()
    d.X, d.Z, d.J, d.F = xg.numel(), zg.numel(), J, F
    d.xstride, d.zstride, d.pa_stride, d.pb_stride = xstride, zstride, sa, sb
    d.dtype, d.device = (_lib.QDAS_F32 if dtype == F32 else _lib.QDAS_F64), -1
    d.xg, d.zg, d.pa, d.pb = (C.c_void_p(t.data_ptr()) for t in (xg, zg, pa, pb))
    d.queue = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    return d


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ---------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("ord", ["ZX", "XZ"])
@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("name", GRIDS)
def test_backprojection_and_column_sums_against_the_restatement(name, F, ord, dtype, monkeypatch):
    """outputs on guarded, poisoned buffers: no guard hit, every element written.  The rays that give nothing in the forward entries (misses, zero length, NaN
    and Inf points) carry a NaN residual: it must not reach the output"""
    c = case(name, dtype)
    rn = c["r"][:F].copy()
    rn[:, c["L"] == 0] = np.nan
    r = dev(rn if F > 1 else rn[0], dtype)
    with GD.guard_outputs(monkeypatch) as gd:
        g, col = RP.ray_backproject(r, c["xg"], c["zg"], dev(c["pa"], dtype), dev(c["pb"], dtype), ord=ord, colsum=True)
        assert gd.check(g, col) == 2
    shape = (c["Z"], c["X"]) if ord == "ZX" else (c["X"], c["Z"])
    assert tuple(g.shape) == ((F,) + shape if F > 1 else shape) and tuple(col.shape) == shape and g.dtype == dtype and col.dtype == dtype
    want = np.einsum("jxz,fj->fxz", c["W"], c["r"][:F])
    eg, ec = rel(xz(g, ord).reshape(F, c["X"], c["Z"]), want), rel(xz(col, ord), c["W"].sum(0))
    print(f"raypaths backproject {name} F={F} {ord} {dtype}: J={c['J']} g {eg:.3e} colsum {ec:.3e}")
    assert eg <= TOL["g", dtype] and ec <= TOL["g", dtype]
    assert np.isfinite(xz(g, ord)).all(), "the r[j] of a ray that gives nothing reached the output"
    assert (xz(col, ord) >= 0).all() and (xz(col, ord)[c["W"].sum(0) == 0] == 0).all()


@pytest.mark.parametrize("J", [1, 63, 64, 65, 129])
def test_ray_counts_around_the_chunk_of_64(J):
    dtype = F64
    c = case("11x9", dtype)
    sel = (7 * np.arange(J)) % c["J"]
    r = _rnd(np.random.default_rng(J).standard_normal(J), dtype)
    g, col = RP.ray_backproject(dev(r, dtype), c["xg"], c["zg"], c["pa"][:, sel], c["pb"][:, sel], ord="XZ", colsum=True)
    live = c["L"][sel] > 0
    want = np.einsum("jxz,j->xz", c["W"][sel][live], r[live])
    scale = max(np.abs(want).max(), c["W"].max())
    assert np.abs(xz(g, "XZ") - want).max() <= TOL["g", dtype] * scale and np.abs(xz(col, "XZ") - c["W"][sel].sum(0)).max() <= TOL["g", dtype] * scale


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_point_strides_of_zero_broadcast_one_point(dtype):
    c = case("33x41", dtype)
    one = c["pa"][:, 12:13]
    ref = R.dense_many(c["xg"], c["zg"], one, c["pb"])
    r = dev(c["r"][0], dtype)
    for pa, pb in ((one, c["pb"]), (c["pb"], one), (one[:, 0], c["pb"])):
        g = RP.ray_backproject(r, c["xg"], c["zg"], pa, pb, ord="XZ")
        e = rel(xz(g, "XZ"), np.einsum("jxz,j->xz", ref, c["r"][0]))
        print(f"raypaths backproject, one point against many {dtype}: {e:.3e}")
        assert e <= TOL["g", dtype]


# ---------------------------------------------------------------------------------------------------------------- the adjoint identity
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["11x9", "33x41", "17x7"])
def test_adjoint_identity_with_the_devices_own_forward(name, dtype):
    """|<A s, r> - <s, A' r>| <= c eps <A |s|, |r|>, the inner products taken in float64 on the host from what the two entries returned"""
    c = case(name, dtype)
    rng = np.random.default_rng(5)
    s = _rnd(rng.standard_normal((c["X"], c["Z"])), dtype)
    live = c["L"] > 0                                                         # (a NaN ray's y is 0 and its r is not looked at: the pairs agree on it)
    r = c["r"][0]
    sd = dev(s, dtype)
    y, _ = RP.ray_integrals(sd, c["xg"], c["zg"], c["pa"], c["pb"], ord="XZ")
    ya, _ = RP.ray_integrals(sd.abs(), c["xg"], c["zg"], c["pa"], c["pb"], ord="XZ")
    g = RP.ray_backproject(dev(r, dtype), c["xg"], c["zg"], c["pa"], c["pb"], ord="XZ")
    lhs = float(np.dot(y.cpu().numpy().astype(np.float64)[live], r[live]))
    rhs = float(np.sum(s * xz(g, "XZ")))
    scale = float(np.dot(ya.cpu().numpy().astype(np.float64)[live], np.abs(r[live])))
    cst = abs(lhs - rhs) / (EPS[dtype] * scale)
    print(f"adjoint identity {name} {dtype}: <As, r> = {lhs:.6e}, <s, A'r> = {rhs:.6e}, c = {cst:.3f}")
    assert cst <= TOL["adj", dtype]


# ---------------------------------------------------------------------------------------------------------------- exact properties
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_rays_along_grid_lines_back_project_onto_that_line_only(dtype):
    """exact zeros beside the line: an event puts the point ON the grid value, so the neighbours' hats are 0 there -- in the last row and column too"""
    c = case("33x41", dtype)
    xg, zg = c["xg"], c["zg"]
    X, Z = xg.size, zg.size
    cols, rows = [0, 7, 8, X - 1], [0, 20, 24, Z - 1]
    for i in cols:
        g, col = RP.ray_backproject(dev([2.5], dtype), xg, zg, [xg[i], zg[0]], [xg[i], zg[-1]], ord="XZ", colsum=True)
        g, col = xz(g, "XZ"), xz(col, "XZ")
        assert (np.delete(g, i, axis=0) == 0).all() and (np.delete(col, i, axis=0) == 0).all() and (col[i] > 0).all()
        assert abs(col[i].sum() - (zg[-1] - zg[0])) <= TOL["g", dtype] * Z * (zg[-1] - zg[0])
    for k in rows:
        g, col = RP.ray_backproject(dev([2.5], dtype), xg, zg, [xg[-1], zg[k]], [xg[0], zg[k]], ord="XZ", colsum=True)
        g, col = xz(g, "XZ"), xz(col, "XZ")
        assert (np.delete(g, k, axis=1) == 0).all() and (np.delete(col, k, axis=1) == 0).all() and (col[:, k] > 0).all()
        assert abs(col[:, k].sum() - (xg[-1] - xg[0])) <= TOL["g", dtype] * X * (xg[-1] - xg[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_unit_residuals_give_the_column_sums_bit_for_bit(dtype):
    c = case("33x41", dtype)
    inside = slice(40, 50)                                                    # raypaths_ref.rays: the ten rays wholly inside the grid
    pa, pb = c["pa"][:, inside], c["pb"][:, inside]
    assert (pa[0] >= c["xg"][0]).all() and (pb[0] <= c["xg"][-1]).all() and (c["L"][inside] > 0).all()
    g, col = RP.ray_backproject(torch.ones(10, dtype=dtype, device="cuda"), c["xg"], c["zg"], pa, pb, colsum=True)
    assert ST.same_bits(g, col) and float(col.sum()) > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_one_nan_reaches_exactly_the_nodes_its_ray_weighs(dtype):
    c = case("33x41", dtype)
    j = 43                                                                    # a random ray wholly inside the grid: it goes through no node
    r = c["r"][0].copy()
    r[~np.isfinite(r)] = 0
    base = RP.ray_backproject(dev(r, dtype), c["xg"], c["zg"], c["pa"], c["pb"], ord="XZ")
    r[j] = np.nan
    got = RP.ray_backproject(dev(r, dtype), c["xg"], c["zg"], c["pa"], c["pb"], ord="XZ")
    nan = np.isnan(xz(got, "XZ"))
    w = c["W"][j]
    assert nan.any() and (w[nan] > 0).all(), "a NaN on a node the restatement gives the ray no weight"
    assert nan[w > TOL["g", dtype] * c["W"].max()].all(), "a node the ray weighs did not see the NaN"
    assert torch.equal(ST.bits(got)[torch.from_numpy(~nan).cuda()], ST.bits(base)[torch.from_numpy(~nan).cuda()]), "a node the ray does not weigh changed"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_two_runs_give_the_same_bits(dtype):
    c = case("33x41", dtype)
    r = dev(c["r"], dtype)
    a = RP.ray_backproject(r, c["xg"], c["zg"], c["pa"], c["pb"], colsum=True)
    b = RP.ray_backproject(r, c["xg"], c["zg"], c["pa"], c["pb"], colsum=True)
    assert ST.same_bits(a[0], b[0]) and ST.same_bits(a[1], b[1])
    # ... and a vector's map does not depend on its companions: the row of one launch is the lone launch
    lone = RP.ray_backproject(r[1], c["xg"], c["zg"], c["pa"], c["pb"])
    assert ST.same_bits(a[0][1], lone)


# ---------------------------------------------------------------------------------------------------------------- the C entry: strides, empty problems
def test_a_strided_view_of_a_larger_array_leaves_the_elements_between_untouched():
    dtype = F64
    c = case("17x7", dtype)
    X, Z, J = c["X"], c["Z"], c["J"]
    xg, zg, a, b, r = dev(c["xg"], dtype), dev(c["zg"], dtype), dev(c["pa"].T, dtype), dev(c["pb"].T, dtype), dev(c["r"][:2], dtype)
    gd = GD.Guard()
    big, bigc = gd.empty((2, 2 * Z, 3 * X), dtype, "cuda"), gd.empty((2 * Z, 3 * X), dtype, "cuda")
    # node (ix, iz) of map f at big[f, 2 iz, 1 + 3 ix]: the maps are NOT X Z elements apart in such an array, so one call per map
    for f in range(2):
        d = desc(xg, zg, a, b, J, dtype, F=1, xstride=3, zstride=2 * 3 * X)
        _lib.check(_lib.lib().qdas_raypaths_backproject(C.byref(d), ptr(r[f]), ptr(big[f, 0, 1:]), ptr(bigc[0, 1:]) if f == 0 else None))
    gd.check()
    want = RP.ray_backproject(r, c["xg"], c["zg"], c["pa"], c["pb"], colsum=True)
    assert ST.same_bits(big[:, ::2, 1::3].contiguous(), want[0]) and ST.same_bits(bigc[::2, 1::3].contiguous(), want[1])
    mask = torch.ones(big.shape[1:], dtype=torch.bool, device="cuda")
    mask[::2, 1::3] = False
    assert bool((ST.bits(big)[:, mask] == -1).all()) and bool((ST.bits(bigc)[mask] == -1).all()), "an element between the view's was written"          # (all-0xFF)


def test_no_vectors_and_no_rays():
    """F = 0: a non-NULL colsum is the whole job, r and g may be NULL.  J = 0 writes zeros (the points and r may be NULL)"""
    dtype = F32
    c = case("9x9", dtype)
    X, Z, J = c["X"], c["Z"], c["J"]
    xg, zg, a, b = dev(c["xg"], dtype), dev(c["zg"], dtype), dev(c["pa"].T, dtype), dev(c["pb"].T, dtype)
    L = _lib.lib()
    col = GD.guarded_empty((Z, X), dtype, "cuda")
    _lib.check(L.qdas_raypaths_backproject(C.byref(desc(xg, zg, a, b, J, dtype, F=0, xstride=1, zstride=X)), None, None, ptr(col)))
    GD.check(col)
    assert ST.same_bits(col, RP.ray_backproject(dev(c["r"][0], dtype), c["xg"], c["zg"], c["pa"], c["pb"], colsum=True)[1])
    g, col = GD.guarded_empty((2, Z, X), dtype, "cuda"), GD.guarded_empty((Z, X), dtype, "cuda")
    d = desc(xg, zg, a, b, 0, dtype, F=2, xstride=1, zstride=X)
    d.pa = d.pb = None
    _lib.check(L.qdas_raypaths_backproject(C.byref(d), None, ptr(g), ptr(col)))
    GD.check(g, col)
    assert not g.any() and not col.any()
    # the Python layer: shapes of empty problems
    g, col = RP.ray_backproject(torch.zeros((0, J), dtype=dtype, device="cuda"), c["xg"], c["zg"], c["pa"], c["pb"], colsum=True)
    assert tuple(g.shape) == (0, Z, X) and float(col.sum()) > 0
    g = RP.ray_backproject(torch.zeros((2, 0), dtype=dtype, device="cuda"), c["xg"], c["zg"], np.zeros((2, 0)), np.zeros((2, 0)), ord="XZ")
    assert tuple(g.shape) == (2, X, Z) and not g.any()


def test_python_refusals_on_the_device():
    x, z = np.arange(4.0), np.arange(5.0)
    with pytest.raises(DasError, match="3 values per vector for 2 rays"):
        RP.ray_backproject(torch.zeros(3, device="cuda"), x, z, np.zeros((2, 2)), np.ones((2, 2)))
    with pytest.raises(DasError, match="monotonic"):
        RP.ray_backproject(torch.zeros(1, device="cuda"), torch.tensor([0.0, 2.0, 1.0, 3.0], device="cuda"), z, [0, 0], [1, 1])
    s0 = torch.full((5, 4), 1 / 1540.0, device="cuda")
    with pytest.raises(DasError, match="4 x 5"):
        RP.ray_sart(torch.zeros(1, device="cuda"), x, z, [0, 0], [1, 1], s0, ord="XZ")
    with pytest.raises(DasError, match="2 arrival times for 1 rays"):
        RP.ray_sart(torch.zeros(2, device="cuda"), x, z, [0, 0], [1, 1], s0)
    out = RP.ray_sart(torch.zeros(1, device="cuda"), x, z, [0, 0], [1, 1], s0, iters=0)
    assert ST.same_bits(out, s0) and out.data_ptr() != s0.data_ptr()
    assert qups_amd.ray_sart is RP.ray_sart and qups_amd.ray_backproject is RP.ray_backproject


# ---------------------------------------------------------------------------------------------------------------- the stream case
@contextlib.contextmanager
def own_stream():
    """a non-blocking stream that exists for this test only.  Every live stream holds one of the process's few hardware queues (the runtime hands a new stream
    the least used one), and torch's pool streams live as long as the process: one more ``torch.cuda.Stream()`` here would move every stream a later test file
    makes onto another queue -- beside another neighbour, the null stream among them -- and tests/test_gpu_streams.py times wrappers that wait for the null stream.
    So the stream is created through the HIP runtime libqdas.so is linked against (the process's only one) and destroyed at the end: the suite's streams stay
    where they were."""
    L = _lib.lib()
    create, destroy = L.hipStreamCreateWithFlags, L.hipStreamDestroy
    create.argtypes, destroy.argtypes = [C.POINTER(C.c_void_p), C.c_uint], [C.c_void_p]
    h = C.c_void_p()
    assert create(C.byref(h), 1) == 0 and h.value                           # hipStreamNonBlocking
    try:
        yield torch.cuda.ExternalStream(h.value)
    finally:
        torch.cuda.synchronize()
        assert destroy(h) == 0


def test_stream_delayed_producer_on_a_side_stream():
    """grid, points and residuals are all-0xFF twins that receive the true data on a non-blocking side stream behind FILL_MS of fills; the entry, issued on that
    stream, and clones taken directly behind it give the serial result bit for bit, and the wrapper returns while the filler is still running"""
    dtype = F32
    c = case("33x41", dtype)
    xg, zg, a, b = dev(c["xg"], dtype), dev(c["zg"], dtype), dev(c["pa"].T, dtype), dev(c["pb"].T, dtype)
    r = dev(np.nan_to_num(c["r"]), dtype)
    J, X, Z = c["J"], c["X"], c["Z"]

    def fn(xg, zg, a, b, r):
        g = torch.empty((3, Z, X), dtype=dtype, device="cuda")
        col = torch.empty((Z, X), dtype=dtype, device="cuda")
        RP._backproject_into(g, col, r, xg, zg, a, b, J, 1, 1, dtype, xg.device, 1, X)
        return g, col

    want = fn(xg, zg, a, b, r)
    torch.cuda.synchronize()
    with own_stream() as side:
        with torch.cuda.stream(side):                                        # warm: allocator blocks of this stream, code objects
            fn(xg, zg, a, b, r)
        torch.cuda.synchronize()
        got, clones, early = ST.run_delayed(fn, [xg, zg, a, b, r], side, FILL_MS)
    for g, cl, wt in zip(got, clones, want):
        assert ST.same_bits(g, wt) and ST.same_bits(cl, wt)
    assert early, "the wrapper did not return before the queued work had run: it waits for the stream (or for the device)"
    assert np.isfinite(want[0].cpu().numpy()).all() and float(want[1].sum()) > 0


# ---------------------------------------------------------------------------------------------------------------- SART
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["11x9", "33x41"])
def test_sart_against_the_numpy_iteration_on_the_dense_matrix(name, dtype):
    """the host test's grids, rays and medium; the device after 1 and 10 steps against numpy on the restatement's float64 matrix (for float32 the matrix of the
    rounded grid and points and the rounded arrival times), and in float64 the R-weighted residual of the device's own iterates does not increase"""
    c = S.case(name)
    xg, zg, pa, pb, t, s0 = (_rnd(c[k], dtype) for k in ("xg", "zg", "pa", "pb", "t", "s0"))
    A = c["A"] if dtype == F64 else R.dense_many(xg, zg, pa, pb).reshape(pa.shape[1], -1)
    maps, _ = S.sart(A, t, s0, 10)
    X, Z = c["X"], c["Z"]
    s0d, td = dev(s0.reshape(X, Z), dtype), dev(t, dtype)
    keep = s0d.clone()
    res = []
    for k in range(11):
        s = RP.ray_sart(td, xg, zg, pa, pb, s0d, iters=k, ord="XZ")
        assert tuple(s.shape) == (X, Z) and s.dtype == dtype
        sk = s.cpu().numpy().astype(np.float64).reshape(-1)
        e = t - A @ sk
        res.append(float(np.sqrt(np.sum(e * e / A.sum(1)))))
        if k in (1, 10):
            err = rel(sk, maps[k])
            print(f"ray_sart {name} {dtype} after {k} steps: {err:.3e} of the largest slowness; weighted residual {res[0]:.3e} -> {res[-1]:.3e}")
            assert err <= TOL["sart", dtype]
    assert ST.same_bits(s0d, keep), "ray_sart modified its start"
    if dtype == F64:
        assert all(b <= a for a, b in zip(res, res[1:])) and res[-1] < res[0]
    zx = RP.ray_sart(td, xg, zg, pa, pb, s0d.t().contiguous(), iters=3, relax=0.7)
    assert tuple(zx.shape) == (Z, X) and ST.same_bits(zx.t().contiguous(), RP.ray_sart(td, xg, zg, pa, pb, s0d, iters=3, relax=0.7, ord="XZ"))


def test_arrival_times_to_a_map_the_eikonal_solver_accepts():
    """end to end on a 32-element array over a 32 x 32 map: travel times through a two-layer medium from ray_integrals, 10 SART steps from the homogeneous map,
    and the eikonal travel-time tables of the result are finite.  (Recovery of the layers is not asserted: one aperture does not determine the map.)"""
    from qups_amd import eikonal as E
    dtype = F64
    n, dp = 32, 0.5e-3
    xg = zg = dp * np.arange(n)
    c_true = np.where(zg[None, :] > 8e-3, 1600.0, 1500.0) * np.ones((n, 1))                     # X x Z
    ie, ib = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")                            # every element (top) to every node of the bottom row
    pa = np.stack((xg[ie.ravel()], np.full(n * n, zg[0])))
    pb = np.stack((xg[ib.ravel()], np.full(n * n, zg[-1])))
    t, ln = RP.ray_integrals(dev(1 / c_true, dtype), xg, zg, pa, pb, ord="XZ")
    assert bool((ln > 0).all())
    s = RP.ray_sart(t, xg, zg, pa, pb, torch.full((n, n), 1 / 1540.0, dtype=dtype, device="cuda"), iters=10, ord="XZ")
    sn = s.cpu().numpy()
    assert np.isfinite(sn).all() and (sn > 1 / 1700.0).all() and (sn < 1 / 1400.0).all()
    y, _ = RP.ray_integrals(s, xg, zg, pa, pb, ord="XZ")
    y0, _ = RP.ray_integrals(torch.full_like(s, 1 / 1540.0), xg, zg, pa, pb, ord="XZ")
    assert float(torch.linalg.vector_norm(t - y)) < 0.2 * float(torch.linalg.vector_norm(t - y0))
    i, k = np.meshgrid(np.arange(n) + 1.0, np.arange(n) + 1.0, indexing="ij")
    Pi = np.stack([i.ravel(order="F"), k.ravel(order="F")])
    src = np.stack([np.arange(n) + 1.0, np.ones(n)])
    tau = E.travel_time_tables(1 / s, dp, src, Pi, (n, n, 1))
    tn = tau.cpu().numpy()
    assert tn.shape == (n, n, 1, n) and np.isfinite(tn).all() and (tn >= 0).all() and tn.max() > (n - 1) * dp / 1700.0
