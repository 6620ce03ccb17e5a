"""qdas_scanconvert and its Python layer (qups_amd/scanconvert.py, Scan.scanConvert) on the device, against the float64 restatement tests/scanconvert_ref.py,
the closed form of a linear field and exact node hits.

Grids (tests/scanconvert_ref.py): four polar (2 x 2 -> 7 x 5, 5 x 4 non-uniform -> 23 x 19, 17 x 9 non-uniform -> 70 x 65, 64 x 33 uniform -> 130 x 129) and
three spherical (2 x 2 x 2 -> 5^3, 5 x 4 x 3 non-uniform -> 13 x 11 x 9, 17 x 9 x 8 -> 33 x 31 x 29) with the C5 sector; every query keeps 1e-9 of an axis
span from the sector's boundary (asserted where the cases are built), so the inside mask must be IDENTICAL to the restatement's.

TOLERANCE on inside pixels: |out - ref| <= K (eps_dtype + eps64 G) max|v|, G = the largest max|axis| / min cell width of the source axes (float64 geometry
rounding enters through the slope across a cell), v the corner values after pre.  MEASURED holds the largest ratio seen over every case of this file per
precision and pre; K is 4 x that, rounded up (the margin for other boxes' math library rounding), and may in no case exceed 64: seven lerps of a few roundings
each do not need more, and anything larger would hide a misplaced weight.  The data are random normal, so a wrong cell is an error of the order of max|b|.

This file also holds the entry's STREAM CASES (``STREAM_CASES``): it takes its stream in the descriptor's ``queue`` field, because the census of ``void
*stream`` parameters (tests/test_streams_host.py) is a pinned list."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from qups_amd import DasError, Scan, Sequence, Transducer, UltrasoundSystem, _lib
from qups_amd import scanconvert as SC
from tests import guards as GD
from tests import scanconvert_ref as R
from tests import streams as ST

pytestmark = pytest.mark.gpu

MEASURED = {(32, "none"): 0.941, (32, "abs"): 0.932, (32, "db"): 0.668, (64, "none"): 0.758, (64, "abs"): 0.506, (64, "db"): 0.605}      # MI355X, every case below
K = {k: min(64.0, float(np.ceil(4 * v))) for k, v in MEASURED.items()}
STREAM_CASES = ("test_stream_delayed_producer_on_a_side_stream", "test_stream_source_rewritten_right_after_the_call")
FILL_MS = 60
DT = {"f32": np.float32, "f64": np.float64, "c64": np.complex64, "c128": np.complex128}
TD = {np.float32: torch.float32, np.float64: torch.float64, np.complex64: torch.complex64, np.complex128: torch.complex128}
QNAN = {4: 0x7FC00000, 8: 0x7FF8000000000000}
SEEN = {}


def bits_of(dt):
    return 32 if np.dtype(dt) in (np.dtype(np.float32), np.dtype(np.complex64)) else 64


def real_of(dt):
    return np.float32 if bits_of(dt) == 32 else np.float64


def case_of(name):
    return R.polar_case(name) if name in R.POLAR else R.spherical_case(name)


@functools.lru_cache(maxsize=None)
def problem(name, dtname, pre):
    """the data (3 pages, the values the device sees; exact zeros planted for db) and the restatement's result with NaN outside -- computed once, never modified"""
    c = case_of(name)
    shape = tuple(c[k].size for k in (("r", "a", "e") if "e" in c else ("r", "a"))) + (3,)
    b = R.data(shape, DT[dtname], 11, zeros=5 if pre == "db" else 0)
    floor = -120.0 if pre == "db" else -np.inf
    wide = b.astype(np.complex128 if np.iscomplexobj(b) else np.float64)
    if "e" in c:
        want, inside = R.convert_spherical(wide, c["r"], c["a"], c["e"], c["origin"], c["x"], c["y"], c["z"], pre=pre, db_floor=floor)
    else:
        want, inside = R.convert_polar(wide, c["r"], c["a"], c["origin"], c["x"], c["z"], pre=pre, db_floor=floor)
    for v in (b, want, inside):
        v.setflags(write=False)
    return c, b, floor, want, inside


def dev_axes(c):
    """the axes as the C ABI takes them: float64 device vectors, angles in radians"""
    names = ("r", "a", "e", "x", "y", "z") if "e" in c else ("r", "a", "x", "z")
    return {k: torch.from_numpy(np.array(c[k])).cuda() for k in names}


def dev_data(b):
    """R fastest in memory, like the view DAS returns"""
    return torch.from_numpy(np.array(b, order="F")).cuda()


def raw(c, ax, bt, pre="none", db_floor=-np.inf, fill=np.nan, guard=None, stream=None):
    """the C entry on a guarded, poisoned output; ``bt``: a device tensor R x A [x E] x P with any strides.  Returns the output, Z x X [x Y] x P, Z fastest."""
    nd = 3 if "e" in c else 2
    P = bt.shape[nd]
    cplx = bt.is_complex()
    odt = bt.dtype if pre == "none" else {torch.complex64: torch.float32, torch.complex128: torch.float64}.get(bt.dtype, bt.dtype)
    oshape = (c["z"].size, c["x"].size) + ((c["y"].size,) if nd == 3 else ()) + (P,)
    g = guard or GD.Guard()
    out = g.empty(tuple(reversed(oshape)), odt, "cuda").permute(*reversed(range(len(oshape))))
    d = _lib.ScanconvertDesc()
    d.R, d.A, d.E = c["r"].size, c["a"].size, (c["e"].size if nd == 3 else 0)
    d.Z, d.X, d.Y, d.P = c["z"].size, c["x"].size, (c["y"].size if nd == 3 else 0), P
    d.sr, d.sa, d.se, d.sp = bt.stride(0), bt.stride(1), (bt.stride(2) if nd == 3 else 0), bt.stride(nd)
    d.dtype = _lib.QDAS_F32 if bt.dtype in (torch.float32, torch.complex64) else _lib.QDAS_F64
    d.cplx, d.pre, d.device = int(cplx), SC.PRE[pre], -1
    d.origin[0], d.origin[1], d.origin[2] = c["origin"]
    d.fill, d.db_floor = fill, db_floor
    for k, t in ax.items():
        setattr(d, k, C.c_void_p(t.data_ptr()))
    d.queue = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    _lib.check(_lib.lib().qdas_scanconvert(C.byref(d), C.c_void_p(bt.data_ptr()), C.c_void_p(out.data_ptr())))
    if guard is None:
        assert g.check(out) == 1, "guard bands intact, every output element written (the fill NaN is not the poison pattern)"
    return out


def check_outside(out, inside, fill):
    """outside the sector every page holds exactly ``fill`` -- NaN: the canonical quiet NaN; complex: fill + 0i"""
    o = out.cpu().numpy()
    o = o[~inside]
    parts = (o.real, o.imag) if np.iscomplexobj(o) else (o,)
    re = np.ascontiguousarray(parts[0])
    if fill != fill:
        assert (re.view(np.uint32 if re.itemsize == 4 else np.uint64) == QNAN[re.itemsize]).all(), "outside is the canonical quiet NaN"
    else:
        assert (re == fill).all()
    if len(parts) == 2:
        assert (parts[1] == 0).all() and not np.signbit(parts[1]).any()


def check_inside(out, want, inside, c, b, dtname, pre, floor, what):
    o = out.cpu().numpy()
    got_mask = ~np.isnan(o.real if np.iscomplexobj(o) else o).any(axis=-1)
    assert np.array_equal(got_mask, inside), f"{what}: the inside mask differs from the restatement's in {np.count_nonzero(got_mask != inside)} pixels"
    bits = bits_of(DT[dtname])
    unit = R.bound(1.0, real_of(DT[dtname]), c, b, pre, floor)
    err = float(np.abs(o[inside] - want[inside][..., :o.shape[-1]]).max()) if inside.any() else 0.0
    SEEN[bits, pre] = max(SEEN.get((bits, pre), 0.0), err / unit)
    print(f"scanconvert {what}: {err / unit:.3f} of (eps + eps64 G) max|v|  (largest so far for {bits, pre}: {SEEN[bits, pre]:.3f}, K = {K[bits, pre]:g})")
    assert err <= K[bits, pre] * unit, f"{what}: {err / unit:.2f} units, K = {K[bits, pre]}"


# ---------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("pre", ["none", "abs", "db"])
@pytest.mark.parametrize("dtname", list(DT))
@pytest.mark.parametrize("name", list(R.POLAR) + list(R.SPHERICAL))
def test_parity_with_the_restatement(name, dtname, pre):
    """pages 1 and 3, fill NaN and 0: the mask identical, outside exactly fill, inside within K units; guard bands intact and no element unwritten"""
    c, b, floor, want, inside = problem(name, dtname, pre)
    ax = dev_axes(c)
    for P in (1, 3):
        bt = dev_data(b[..., :P])
        out = raw(c, ax, bt, pre, floor)
        assert out.shape[-1] == P and out.stride(0) == 1
        check_outside(out, inside, np.nan)
        check_inside(out, want, inside, c, b, dtname, pre, floor, f"{name} {dtname} {pre} P={P}")
        out0 = raw(c, ax, bt, pre, floor, fill=0.0)
        check_outside(out0, inside, 0.0)
        assert ST.same_bits(out0[torch.from_numpy(inside).cuda()], out[torch.from_numpy(inside).cuda()])


def test_the_constants_of_this_file():
    assert all(v <= 64 for v in K.values()) and set(K) == {(b, p) for b in (32, 64) for p in ("none", "abs", "db")}


# ---------------------------------------------------------------------------------------------------------------- closed form, node hits, cell search
@pytest.mark.parametrize("name", list(R.POLAR) + list(R.SPHERICAL))
def test_a_linear_field_is_reproduced(name):
    """float64: c0 + c1 r + c2 a (+ c3 e) on the nodes comes back as that expression of (rho, alpha, eps) at every inside pixel, on non-uniform axes too"""
    c = case_of(name)
    k = [0.3, 1.7 / np.ptp(c["r"]), -0.9 / np.ptp(c["a"])] + ([0.6 / np.ptp(c["e"])] if "e" in c else [])
    f = R.linear_field(k, c["r"], c["a"], c.get("e"))[..., None]
    out = raw(c, dev_axes(c), dev_data(f)).cpu().numpy()[..., 0]
    if "e" in c:
        rho, alpha, eps = R.spherical_coords(c["origin"], c["x"], c["y"], c["z"])
        want = k[0] + k[1] * rho + k[2] * alpha + k[3] * eps
        inside = R.locate(c["r"], rho)[0] & R.locate(c["a"], alpha)[0] & R.locate(c["e"], eps)[0]
    else:
        rho, alpha = R.polar_coords(c["origin"], c["x"], c["z"])
        want = k[0] + k[1] * rho + k[2] * alpha
        inside = R.locate(c["r"], rho)[0] & R.locate(c["a"], alpha)[0]
    assert np.array_equal(~np.isnan(out), inside)
    err = np.abs(out - want)[inside].max()
    unit = R.bound(1.0, np.float64, c, f)
    print(f"scanconvert linear field {name}: {err / unit:.3f} units")
    assert err <= K[64, "none"] * unit


@pytest.mark.parametrize("dtname", ["f64", "f32", "c128"])
def test_node_hits_are_bit_exact(dtname, monkeypatch):
    """in the column x = ox the coordinates are exact: the output there is the source's node values bit for bit, r[0] and r[R-1] included; with both cell searches"""
    c = R.node_hit_case()
    b = np.round(100 * R.data((c["r"].size, c["a"].size, 2), DT[dtname], 3)).astype(DT[dtname])
    ax = dev_axes(c)
    for env in (None, "1"):
        if env:
            monkeypatch.setenv("QDAS_SCANCONVERT_BISECT", env)
        out = raw(c, ax, dev_data(b)).cpu().numpy()
        col = out[:, c["col"], :]
        assert not np.isnan(col[c["rows"]]).any() and np.isnan(col[0]).all() and np.isnan(col[-1]).all(), "r[0] and r[R-1] are inside, their neighbours are not"
        assert np.array_equal(col[c["rows"]], b[:, c["l0"], :])
        want, inside = R.convert_polar(b.astype(np.complex128 if np.iscomplexobj(b) else np.float64), c["r"], c["a"], c["origin"], c["x"], c["z"])
        assert np.array_equal(~np.isnan(out).any(-1), inside)


@pytest.mark.parametrize("name", ["64x33", "17x9x8"])
def test_uniform_fast_path_against_bisection(name, monkeypatch):
    """the same uniform axes once as they are, once with one interior node moved by 1 ulp, once with the bisection forced (QDAS_SCANCONVERT_BISECT=1):
    identical masks; the forced bisection names the same cells, so the same bits; the moved node agrees within the tolerance"""
    c, b, floor, want, inside = problem(name, "f64", "none")
    assert c["uniform"]
    bt = dev_data(b)
    out = raw(c, dev_axes(c), bt)
    c2 = dict(c)
    r2 = np.array(c["r"])
    r2[r2.size // 2] = np.nextafter(r2[r2.size // 2], np.inf)
    c2["r"] = r2
    out2 = raw(c2, dev_axes(c2), bt)
    monkeypatch.setenv("QDAS_SCANCONVERT_BISECT", "1")
    out3 = raw(c, dev_axes(c), bt)
    monkeypatch.delenv("QDAS_SCANCONVERT_BISECT")
    assert ST.same_bits(out3, out)
    m = torch.from_numpy(inside).cuda()
    assert np.array_equal(~np.isnan(out2.cpu().numpy()).any(-1), inside)
    assert float((out2[m] - out[m]).abs().max()) <= R.bound(K[64, "none"], np.float64, c, b)
    check_inside(out, want, inside, c, b, "f64", "none", floor, f"{name} fast path")
    # a non-uniform axis through both searches too
    cn, bn, _, _, _ = problem("17x9", "f64", "none")
    o1 = raw(cn, dev_axes(cn), dev_data(bn))
    monkeypatch.setenv("QDAS_SCANCONVERT_BISECT", "1")
    assert ST.same_bits(raw(cn, dev_axes(cn), dev_data(bn)), o1)


def test_axes_at_the_lds_limit():
    """R + A = 8192 float64 nodes fill the 64 KiB of LDS the entry allows: the launch is taken and the result is right (the source is one column read with an
    angle stride of 0, so the data stay small); one node more is refused before any launch"""
    base = R.polar_case("5x4")
    n = 4096
    c = dict(r=np.linspace(R.R0, R.R1, n), a=R.deg2rad(np.linspace(-R.AMAX, R.AMAX, n)), origin=R.ORIGIN, x=base["x"], z=base["z"])
    col = R.data((n, 1, 1), np.float32, 21)
    b = np.broadcast_to(col, (n, n, 1))
    want, inside = R.convert_polar(b.astype(np.float64), c["r"], c["a"], c["origin"], c["x"], c["z"])
    assert np.array_equal(inside, problem("5x4", "f32", "none")[4]), "the sector's ends are those of the 5x4 case: its margin holds here"
    bt = torch.from_numpy(col).cuda().expand(n, n, 1)
    assert bt.stride() == (1, 0, 1)
    out = raw(c, dev_axes(c), bt)
    check_inside(out, want, inside, c, b, "f32", "none", -np.inf, "LDS limit")
    c2 = dict(c)
    c2["r"] = np.linspace(R.R0, R.R1, n + 1)
    with pytest.raises(_lib.QdasError, match="LDS") as ei:
        raw(c2, dev_axes(c2), torch.zeros((n + 1, 1, 1), device="cuda").expand(n + 1, n, 1))
    assert ei.value.code == _lib.QDAS_EUNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------- memory and strides
@pytest.mark.parametrize("name,dtname,pre", [("17x9", "c64", "db"), ("5x4x3", "f64", "none"), ("64x33", "f32", "abs")])
def test_halos_and_strides_do_not_change_a_bit(name, dtname, pre, monkeypatch):
    """the source embedded in NaN, Inf and zero halos; the I1-fastest view DAS returns, a row-major tensor and a page stride with a gap, through the Python
    layer with guarded outputs: all identical to the C entry on the dense column-major source"""
    c, b, floor, want, inside = problem(name, dtname, pre)
    nd = 3 if "e" in c else 2
    bt = dev_data(b)
    base = raw(c, dev_axes(c), bt, pre, floor)
    ax = dev_axes(c)
    for fill in ("nan", "inf", "0"):
        assert ST.same_bits(raw(c, ax, GD.haloed_view(bt, fill), pre, floor), base)
    args = ((c["r"], c["a_deg"], c["e_deg"], c["origin"], c["x"], c["y"], c["z"]) if nd == 3 else (c["r"], c["a_deg"], c["origin"], c["x"], c["z"]))
    conv = SC.scan_convert3 if nd == 3 else SC.scan_convert
    row_major = torch.from_numpy(np.ascontiguousarray(b)).cuda()
    assert row_major.stride(-1) == 1 and row_major.stride(0) != 1
    gap = torch.full((5,) + tuple(reversed(b.shape[:nd])), float("nan"), dtype=TD[DT[dtname]], device="cuda")
    gap = gap.permute(*reversed(range(nd + 1)))[..., ::2]                                                          # column-major, every other page
    gap.copy_(bt)
    assert gap.stride(0) == 1 and gap.stride(nd) == 2 * int(np.prod(b.shape[:nd]))
    two = torch.from_numpy(np.asfortranarray(np.stack([b[..., :2], b[..., 1:]], -1))).cuda()                        # pages 2 x 2, column-major: collapses
    for src in (bt, row_major, gap, GD.haloed_view(row_major, "nan")):
        with GD.guard_outputs(monkeypatch) as g:
            got, axes = conv(src, *args, pre=pre, db_floor=floor)
            assert g.check(got) == 1
        assert ST.same_bits(got, base) and got.stride(0) == 1 and len(axes) == 3
    got2, _ = conv(two, *args, pre=pre, db_floor=floor)
    assert tuple(got2.shape) == tuple(base.shape[:-1]) + (2, 2) and ST.same_bits(got2[..., 0, 1], base[..., 1]) and ST.same_bits(got2[..., 1, 1], base[..., 2])
    assert ST.same_bits(got2[..., 0, 0], base[..., 0]) and ST.same_bits(got2[..., 1, 0], base[..., 1])
    two_rm = two.contiguous()                                                                                        # row-major pages: copied once
    assert SC.page_stride(two_rm.shape[nd:], two_rm.stride()[nd:])[1] is None
    assert ST.same_bits(conv(two_rm, *args, pre=pre, db_floor=floor)[0], got2)


def test_the_view_das_returns_is_read_in_place(monkeypatch):
    """the stride pattern of UltrasoundSystem.DAS's result -- I1 x I2 x I3 x F with I1 fastest -- reaches the kernel without a copy"""
    c, b, floor, want, inside = problem("17x9", "c64", "none")
    das_like = torch.from_numpy(np.ascontiguousarray(b.transpose(2, 1, 0)[:, None])).cuda().permute(3, 2, 1, 0)      # R x A x 1 x F, R fastest
    assert tuple(das_like.shape) == (17, 9, 1, 3) and das_like.stride(0) == 1
    seen = []
    L = _lib.lib()

    class Spy:
        def __getattr__(self, n):
            return getattr(L, n)

        def qdas_scanconvert(self, d, bp, op):
            seen.append(bp.value)
            return L.qdas_scanconvert(d, bp, op)

    spy = Spy()
    monkeypatch.setattr(SC._lib, "lib", lambda: spy)
    got, _ = SC.scan_convert(das_like, c["r"], c["a_deg"], c["origin"], c["x"], c["z"])
    assert seen == [das_like.data_ptr()] and tuple(got.shape) == (70, 65, 1, 3)
    check_inside(got[:, :, 0, :], want, inside, c, b, "c64", "none", floor, "DAS view")


def test_python_refusals_and_defaults_on_the_device():
    c, b, floor, want, inside = problem("5x4", "f32", "none")
    bt = dev_data(b)
    with pytest.raises(DasError, match="b is r x a_deg"):
        SC.scan_convert(bt.permute(1, 0, 2), c["r"], c["a_deg"], c["origin"], c["x"], c["z"])
    with pytest.raises(DasError, match="half-precision"):
        SC.scan_convert(bt.half(), c["r"], c["a_deg"], c["origin"], c["x"], c["z"])
    with pytest.raises(DasError, match="the x axis must be finite and strictly increasing"):
        SC.scan_convert(bt, c["r"], c["a_deg"], c["origin"], torch.tensor([0.0, 2.0, 1.0], device="cuda"), c["z"])
    with pytest.raises(DasError, match="pre"):
        SC.scan_convert(bt, c["r"], c["a_deg"], c["origin"], c["x"], c["z"], pre="log")
    got, (x, y, z) = SC.scan_convert(bt, c["r"], c["a_deg"], c["origin"])                       # the enclosing grid: non-uniform r -> 161 points
    assert tuple(got.shape) == (161, 161, 3) and x.size == z.size == 161 and y.size == 1
    empty, _ = SC.scan_convert(bt[..., :0], c["r"], c["a_deg"], c["origin"], c["x"], c["z"])
    assert tuple(empty.shape) == (23, 19, 0)


# ---------------------------------------------------------------------------------------------------------------- streams
def _stream_problem():
    c, b, floor, want, inside = problem("64x33", "c64", "db")
    dev = {k: torch.from_numpy(np.array(c[k])).cuda() for k in ("r", "a_deg", "x", "z")}

    def fn(bt, r, a_deg, x, z):
        return SC.scan_convert(bt, r, a_deg, c["origin"], x, z, pre="db", db_floor=floor, check_grid=False)[0]

    return c, b, floor, want, inside, dev, fn


def test_stream_delayed_producer_on_a_side_stream():
    """data and axes are all-0xFF twins that receive the true values on a non-blocking side stream behind FILL_MS of fills; the call issued at once on that
    stream and a clone taken directly behind it give the serial result bit for bit, and the wrapper returns while the filler is still running"""
    c, b, floor, want, inside, dev, fn = _stream_problem()
    args = [dev_data(b), dev["r"], dev["a_deg"], dev["x"], dev["z"]]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                                            # warm: allocator blocks of this stream, code objects
        fn(*args)
    torch.cuda.synchronize()
    serial = fn(*args)
    torch.cuda.synchronize()
    got, clones, early = ST.run_delayed(fn, args, side, FILL_MS)
    assert ST.same_bits(got[0], serial) and ST.same_bits(clones[0], serial)
    assert early, "the wrapper did not return before the queued work had run: it waits for the stream (or for the device)"
    check_inside(serial, want, inside, c, b, "c64", "db", floor, "stream case")


def test_stream_source_rewritten_right_after_the_call():
    """on a side stream behind a filler: the call, then the source overwritten with NaN on the same stream -- the result is the serial one (the kernel is
    ordered in front of the rewrite; the wrapper keeps no reference to a copy it would read later)"""
    c, b, floor, want, inside, dev, fn = _stream_problem()
    bt = dev_data(b)
    serial = fn(bt, dev["r"], dev["a_deg"], dev["x"], dev["z"])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    ST.filler(side, FILL_MS)
    with torch.cuda.stream(side):
        got = fn(bt, dev["r"], dev["a_deg"], dev["x"], dev["z"])
        bt.fill_(float("nan"))
        dev["r"].fill_(float("nan"))
    torch.cuda.synchronize()
    assert ST.same_bits(got, serial) and torch.isnan(bt.real).all()


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_greens_das_scanconvert_peaks_at_the_scatterer():
    """greens of one scatterer -> DAS on a small polar scan of a 32-element convex array -> Scan.scanConvert(b, pre="db"): the argmax of the Cartesian image
    lies within 1.1 mm of the scatterer, the reference's own criterion (test/BFTest.m:306-316)"""
    fc, c0, radius = 3.7e6, 1500.0, 40e-3
    fs = 4 * fc
    xdc = Transducer.convex(32, radius, 0.5, fc=fc)
    scan = Scan.polar(np.linspace(radius + 10e-3, radius + 20e-3, 81), np.linspace(-8.0, 8.0, 65), origin=(0.0, 0.0, -radius))
    us = UltrasoundSystem(xdc, Sequence("FSA", c0=c0), scan, fs=fs)
    th = np.deg2rad(3.0)
    scat = np.array([[(radius + 15e-3) * np.sin(th)], [0.0], [(radius + 15e-3) * np.cos(th) - radius]])
    t = np.arange(-2.0 / fc, 2.0 / fc, 1 / (4 * fs))
    wv = np.exp(-(t * fc * 1.2) ** 2) * np.exp(2j * np.pi * fc * t)
    chd = us.greens(scat, [1.0], wv, t[0], 4 * fs, R0=c0 / fc, interp="cubic", focus=False)
    b = us.DAS(chd, interp="cubic")
    assert tuple(b.shape[:3]) == (81, 65, 1) and b.stride(0) == 1
    bc, scanC = scan.scanConvert(b, pre="db", db_floor=-120.0)
    x, z = scanC.axes["x"], scanC.axes["z"]
    assert tuple(bc.shape[:2]) == (z.size, x.size) and bc.dtype == torch.float32 and bc.stride(0) == 1
    img = bc.reshape(z.size, x.size).cpu().numpy()
    assert np.isnan(img).any() and np.isfinite(img).any()
    iz, ix = np.unravel_index(np.nanargmax(img), img.shape)
    assert np.hypot(x[ix] - scat[0, 0], z[iz] - scat[2, 0]) <= 1.1e-3, (x[ix], z[iz], scat.ravel())
    pos = scan.positions()
    assert x[0] <= pos[0].min() and x[-1] >= pos[0].max() and z[0] <= pos[2].min() and z[-1] >= pos[2].max()
    again, same = scan.scanConvert(b, scanC, pre="db", db_floor=-120.0)
    assert same is scanC and ST.same_bits(again, bc)
    with pytest.raises(DasError, match="Data must be in order 'RAY'"):
        Scan(scan.positions()).scanConvert(b)


def test_the_largest_ratios_seen():
    """(runs last) prints what the cases above measured, the figures behind MEASURED"""
    print("scanconvert measured ratios:", {k: round(v, 3) for k, v in sorted(SEEN.items())})
    for k, v in SEEN.items():
        assert v <= K[k]
