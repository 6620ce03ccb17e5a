"""Scan conversion without a GPU: the float64 restatement (tests/scanconvert_ref.py) against scipy, the closed form of a linear field and exact node hits;
the enclosing Cartesian grids; the core the device kernels compile (qups_amd/csrc/scanconvert_core.h) built for the host with the sanitizers and compared
with the restatement; the C ABI's validation, which happens before any HIP call; the Python layer's argument handling."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from qups_amd import DasError, Scan, _lib
from qups_amd import geometry as G
from qups_amd import scanconvert as SC
from tests import scanconvert_ref as R
from tests.test_streams_host import stream_entries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
LIN = (0.3, 1.7, -0.9, 0.6)          # c0, c1 ptp(r), c2 ptp(a), c3 ptp(e): every term of the field is of order 1


def _lin(c):
    k = [LIN[0], LIN[1] / np.ptp(c["r"]), LIN[2] / np.ptp(c["a"])]
    return k + [LIN[3] / np.ptp(c["e"])] if "e" in c else k


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", list(R.POLAR))
def test_restatement_polar_against_scipy_and_the_closed_form(name):
    """scipy forms the weighted sum of the four corners, the contract three lerps: a handful of roundings of values of the size of max|b| each, 16 eps;
    the closed form: bilinear interpolation reproduces c0 + c1 rho + c2 alpha up to the rounding of the weights (eps rho / h, times the slope c1 h) and of
    three lerps -- a few eps of the field's size (measured: <= 4 eps on these grids), bound 16 eps max|field|"""
    c = R.polar_case(name)
    assert c["margin"] >= R.MARGIN
    b = R.data((c["r"].size, c["a"].size, 2), np.float64, 1)
    out, inside = R.convert_polar(b, c["r"], c["a"], c["origin"], c["x"], c["z"])
    assert out.shape == (c["z"].size, c["x"].size, 2) and 0.3 <= (~inside).mean() <= 0.6 and np.isnan(out[~inside]).all()
    rho, alpha = R.polar_coords(c["origin"], c["x"], c["z"])
    try:
        from scipy.interpolate import RegularGridInterpolator
    except ImportError:
        RegularGridInterpolator = None
    if RegularGridInterpolator is not None:
        for p in range(2):
            ref = RegularGridInterpolator((c["r"], c["a"]), b[:, :, p], method="linear", bounds_error=False, fill_value=np.nan)(np.stack([rho, alpha], -1))
            assert np.array_equal(np.isnan(ref), ~inside)
            assert np.abs(out[:, :, p] - ref)[inside].max() <= 16 * EPS * np.abs(b).max()
    k = _lin(c)
    f = R.linear_field(k, c["r"], c["a"])[:, :, None]
    got, _ = R.convert_polar(f, c["r"], c["a"], c["origin"], c["x"], c["z"])
    want = k[0] + k[1] * rho + k[2] * alpha
    err = np.abs(got[:, :, 0] - want)[inside].max() / np.abs(want[inside]).max()
    print(f"restatement {name}: margin {c['margin']:.2e}, outside {(~inside).mean():.2f}, linear field {err / EPS:.1f} eps")
    assert err <= 16 * EPS


@pytest.mark.parametrize("name", list(R.SPHERICAL))
def test_restatement_spherical_against_scipy_and_the_closed_form(name):
    """as the polar test, with seven lerps: 32 eps"""
    c = R.spherical_case(name)
    b = R.data((c["r"].size, c["a"].size, c["e"].size, 1), np.float64, 2)
    out, inside = R.convert_spherical(b, c["r"], c["a"], c["e"], c["origin"], c["x"], c["y"], c["z"])
    assert out.shape == (c["z"].size, c["x"].size, c["y"].size, 1) and inside.any() and (~inside).any() and np.isnan(out[~inside]).all()
    rho, alpha, eps = R.spherical_coords(c["origin"], c["x"], c["y"], c["z"])
    try:
        from scipy.interpolate import RegularGridInterpolator
        ref = RegularGridInterpolator((c["r"], c["a"], c["e"]), b[..., 0], method="linear", bounds_error=False, fill_value=np.nan)(np.stack([rho, alpha, eps], -1))
        assert np.array_equal(np.isnan(ref), ~inside) and np.abs(out[..., 0] - ref)[inside].max() <= 32 * EPS * np.abs(b).max()
    except ImportError:
        pass
    k = _lin(c)
    got, _ = R.convert_spherical(R.linear_field(k, c["r"], c["a"], c["e"])[..., None], c["r"], c["a"], c["e"], c["origin"], c["x"], c["y"], c["z"])
    want = k[0] + k[1] * rho + k[2] * alpha + k[3] * eps
    assert np.abs(got[..., 0] - want)[inside].max() <= 32 * EPS * np.abs(want[inside]).max()


def test_restatement_node_hits_are_exact_and_the_end_nodes_are_inside():
    c = R.node_hit_case()
    b = np.round(100 * R.data((c["r"].size, c["a"].size, 2), np.float64, 3))
    out, inside = R.convert_polar(b, c["r"], c["a"], c["origin"], c["x"], c["z"])
    col = inside[:, c["col"]]
    assert col[c["rows"]].all() and not col[0] and not col[-1], "r[0] and r[R-1] are inside, the pixels before and past them are not"
    assert np.array_equal(out[c["rows"], c["col"], :], b[:, c["l0"], :])
    inside1, k, w = R.locate(c["r"], c["r"])
    assert inside1.all() and np.array_equal(k, np.minimum(np.arange(c["r"].size), c["r"].size - 2)) and w[-1] == 1.0 and (w[:-1] == 0).all()
    assert not R.locate(c["r"], np.array([np.nan, np.inf, -np.inf]))[0].any()


def test_restatement_pre_acts_on_the_corners_and_nan_corners_spread():
    c = R.polar_case("5x4")
    b = R.data((5, 4, 1), np.complex128, 4, zeros=3)
    args = (c["r"], c["a"], c["origin"], c["x"], c["z"])
    db, inside = R.convert_polar(b, *args, pre="db", db_floor=-120.0)
    assert np.array_equal(db, R.convert_polar(np.maximum(20 * np.log10(np.maximum(np.abs(b), 1e-300)), -120.0), *args)[0], equal_nan=True)
    assert db[inside].min() >= -120.0 and np.isrealobj(db)
    ab = R.convert_polar(b, *args, pre="abs", fill=0.0)[0]
    assert (ab[~inside] == 0).all() and (ab[inside] >= 0).all()
    raw = R.convert_polar(b, *args, pre="db")[0]
    assert np.isinf(raw[inside]).any() or np.isnan(raw[inside]).any(), "without a floor an exact zero gives -inf corners"
    b2 = b.copy()
    b2[2, 1, 0] = np.nan
    out = R.convert_polar(b2, *args)[0]
    _, k, _ = R.locate(c["r"], R.polar_coords(c["origin"], c["x"], c["z"])[0])
    _, l, _ = R.locate(c["a"], R.polar_coords(c["origin"], c["x"], c["z"])[1])
    touched = inside & (k >= 1) & (k <= 2) & (l >= 0) & (l <= 1)
    assert np.isnan(out[touched]).all() and not np.isnan(out[inside & ~touched]).any()


# ---------------------------------------------------------------------------------------------------------------- the enclosing grid
def _contains(axes, pos):
    return all(ax[0] <= pos[k].min() and ax[-1] >= pos[k].max() for k, ax in enumerate(axes))


def test_enclosing_grid_of_a_polar_scan():
    og = (1e-3, 2e-3, -49.6e-3)
    a = np.linspace(-37, 37, 33)
    r = np.linspace(49.6e-3, 99.6e-3, 64)
    dr = np.diff(r).min()
    x, y, z = G.cartesian_of_polar(r, a, og)
    assert _contains((x, y, z), G.scan_polar(r, a, og))
    for ax in (x, z):
        assert np.allclose(np.diff(ax), dr, rtol=1e-12) and np.abs(ax / dr - np.round(ax / dr)).max() < 1e-9          # multiples of dr
        assert ax.size >= 2
    assert y.size == 2 and y[0] == dr * np.floor(og[1] / dr) and y[0] < og[1] < y[1], "zero extent off a multiple of dr: the two multiples around it"
    y0 = G.cartesian_of_polar(r, a, (1e-3, 0.0, -49.6e-3))[1]
    assert y0.size == 1 and y0[0] == 0.0, "an axis of zero extent is the single value dr floor(min / dr)"
    y5 = G.cartesian_of_polar(r, a, (1e-3, 5 * dr, -49.6e-3))[1]
    assert y5.size == 1 and y5[0] == dr * np.floor(5 * dr / dr) == 5 * dr
    # nearly uniform (within 1e-3): dr is the smallest difference; beyond: the reference's default counts
    rn = r + 4e-4 * dr * np.sin(np.arange(64.0))
    assert G._enclosing_step(rn) == np.diff(rn).min() and np.isfinite(G._enclosing_step(rn))
    x2, y2, z2 = G.cartesian_of_polar(rn, a, og)
    assert np.allclose(np.diff(x2), np.diff(rn).min(), rtol=1e-12) and _contains((x2, y2, z2), G.scan_polar(rn, a, og))
    rv = r ** 1.3 / r[0] ** 0.3
    assert np.isnan(G._enclosing_step(rv)) and np.isinf(G._enclosing_step([1.0]))
    x3, y3, z3 = G.cartesian_of_polar(rv, a, og)
    pos = G.scan_polar(rv, a, og)
    assert x3.size == z3.size == 161 and y3.size == 1 and y3[0] == pos[1].max() and _contains((x3, y3, z3), pos)
    assert x3[0] == pos[0].min() and x3[-1] == pos[0].max() and z3[0] == pos[2].min() and z3[-1] == pos[2].max()
    # a y axis with extent
    x4, y4, z4 = G.cartesian_of_polar(r, a, og, y=(-1e-3, 0.0, 1e-3))
    assert y4.size >= 3 and _contains((x4, y4, z4), G.scan_polar(r, a, og, y=(-1e-3, 0.0, 1e-3)))


def test_enclosing_grid_of_a_spherical_scan_and_its_positions():
    og = (0.0, 1e-3, -5e-3)
    r, a, e = np.linspace(10e-3, 40e-3, 31), np.linspace(-25, 25, 11), np.linspace(-20, 15, 8)
    pos = G.scan_spherical(r, a, e, og)
    assert pos.shape == (3, 31, 11, 8)
    ra, re_ = np.deg2rad(a[3]), np.deg2rad(e[6])
    want = r[20] * np.array([np.cos(re_) * np.sin(ra), np.sin(re_), np.cos(re_) * np.cos(ra)]) + og                   # [Z, X, Y] = sph2cart(A, E, R)
    assert np.allclose(pos[:, 20, 3, 6], want, rtol=1e-15, atol=1e-18)
    assert np.allclose(np.linalg.norm(pos - np.array(og).reshape(3, 1, 1, 1), axis=0), r[:, None, None])
    axes = G.cartesian_of_spherical(r, a, e, og)
    assert _contains(axes, pos) and all(np.allclose(np.diff(ax), 1e-3, rtol=1e-9) for ax in axes)
    two = G.cartesian_of_spherical(r ** 1.2, a, e, og)
    p2 = G.scan_spherical(r ** 1.2, a, e, og)
    assert all(ax.size == 2 for ax in two) and all(ax[0] == p2[k].min() and ax[1] == p2[k].max() for k, ax in enumerate(two))
    s = Scan.spherical(r, a, e, og)
    assert s.size == (31, 11, 8) and s.axes["kind"] == "spherical" and np.array_equal(s.positions(), pos)
    assert Scan(pos).axes is None and Scan.polar(r, a).axes["kind"] == "polar" and Scan.cartesian([0.0, 1.0], [0.0, 1.0]).axes["kind"] == "cartesian"


# ---------------------------------------------------------------------------------------------------------------- the device's core, on the host
@pytest.fixture(scope="module")
def core_exe(tmp_path_factory):
    """scanconvert_core.h under AddressSanitizer and UBSan in a stand-alone program: axes and data are heap blocks of exactly their size"""
    exe = str(tmp_path_factory.mktemp("sc") / "scanconvert_core_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=fast", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "qups_amd", "csrc"), os.path.join(ROOT, "tests", "scanconvert_core_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _fmt(v):
    return " ".join(repr(float(t)) for t in np.asarray(v, np.float64).reshape(-1))


def run_core(exe, tmp_path, b, c, *, bits, pre="none", db_floor=-np.inf, fill=np.nan, bisect=0):
    """``(out, inside, uniform flags)``; ``b``: R x A [x E] x P in the values the program is to see"""
    kind = 3 if "e" in c else 2
    cplx = int(np.iscomplexobj(b))
    e, y = (c["e"], c["y"]) if kind == 3 else (np.zeros(0), np.zeros(0))
    P = b.shape[-1]
    path = str(tmp_path / "case.txt")
    with open(path, "w") as f:
        f.write(f"{kind} {bits} {cplx} {SC.PRE[pre]} {c['r'].size} {c['a'].size} {e.size} {c['z'].size} {c['x'].size} {y.size} {P} {bisect}\n")
        f.write(_fmt(list(c["origin"]) + [fill, db_floor]) + "\n")
        for ax in (c["r"], c["a"], e, c["x"], y, c["z"]):
            f.write(_fmt(ax) + "\n")
        flat = np.asarray(b).reshape(-1, order="F")
        f.write(_fmt(np.stack([flat.real, flat.imag], 1) if cplx else flat) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    flags = tuple(int(v) for v in lines[0].split())
    rows = [ln.split() for ln in lines[1:]]
    shape = (c["z"].size, c["x"].size) + ((y.size,) if kind == 3 else ()) + (P,)
    ins = np.array([int(row[0]) for row in rows], bool).reshape(shape, order="F")
    val = np.array([complex(float.fromhex(row[1]), float.fromhex(row[2])) for row in rows]).reshape(shape, order="F")
    return (val if cplx and pre == "none" else val.real), ins[..., 0], flags


def _ref(b, c, **kw):
    if "e" in c:
        return R.convert_spherical(b, c["r"], c["a"], c["e"], c["origin"], c["x"], c["y"], c["z"], **kw)
    return R.convert_polar(b, c["r"], c["a"], c["origin"], c["x"], c["z"], **kw)


bound = R.bound


@pytest.mark.parametrize("pre", ["none", "abs", "db"])
@pytest.mark.parametrize("dt", [np.float32, np.float64, np.complex64, np.complex128], ids=["f32", "f64", "c64", "c128"])
@pytest.mark.parametrize("name", list(R.POLAR) + list(R.SPHERICAL))
def test_the_core_on_the_host_matches_the_restatement(core_exe, tmp_path, name, dt, pre):
    """same text as the device, same bound as the device test (tests/test_gpu_scanconvert.py K); the inside mask is identical, the outside is exactly fill,
    a uniform axis is found uniform and the forced bisection gives the same cells: the same bits"""
    from tests.test_gpu_scanconvert import K
    c = R.polar_case(name) if name in R.POLAR else R.spherical_case(name)
    shape = tuple(c[k].size for k in (("r", "a", "e") if "e" in c else ("r", "a"))) + (2,)
    b = R.data(shape, dt, 5, zeros=3 if pre == "db" else 0)
    floor = -120.0 if pre == "db" else -np.inf
    real = np.float32 if np.dtype(dt) in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64
    bits = 32 if real is np.float32 else 64
    want, inside = _ref(b.astype(np.complex128 if np.iscomplexobj(b) else np.float64), c, pre=pre, db_floor=floor)
    got, ins, flags = run_core(core_exe, tmp_path, b, c, bits=bits, pre=pre, db_floor=floor)
    assert np.array_equal(ins, inside) and np.isnan(got[~inside]).all()
    err = np.abs(got - want)[inside].max()
    tol = bound(K[bits, pre], real, c, b, pre, floor)
    print(f"host core {name} {np.dtype(dt).name} {pre}: {err / (tol / K[bits, pre]):.2f} of (eps + eps64 G) max|v|")
    assert err <= tol
    assert all(flags[:3 if "e" in c else 2]) == c["uniform"] or name.startswith("2x2")
    got0, ins0, _ = run_core(core_exe, tmp_path, b, c, bits=bits, pre=pre, db_floor=floor, fill=0.0, bisect=1)
    assert np.array_equal(ins0, inside) and (got0[~inside] == 0).all() and np.array_equal(got0[inside], got[inside])


def test_the_core_node_hits_on_the_host_are_exact(core_exe, tmp_path):
    c = R.node_hit_case()
    b = np.round(100 * R.data((c["r"].size, c["a"].size, 2), np.float64, 3))
    for bits in (64, 32):
        for bisect in (0, 1):
            got, ins, flags = run_core(core_exe, tmp_path, b, c, bits=bits, bisect=bisect)
            assert ins[c["rows"], c["col"]].all() and not ins[0, c["col"]] and not ins[-1, c["col"]]
            assert np.array_equal(got[c["rows"], c["col"], :], b[:, c["l0"], :]) and flags[0] == 1


def test_the_core_survives_broken_inputs(core_exe, tmp_path):
    """NaN and Inf coordinates, a query far outside, R = 2, axes with a repeated node, NaN nodes: the program ends without a sanitizer report and with every
    cell inside its axis (it checks that itself); non-finite coordinates are outside"""
    base = R.polar_case("5x4")
    b = R.data((5, 4, 1), np.float64, 6)
    for bits in (64, 32):
        for bad in (np.nan, np.inf, -np.inf, 1e300, -1e300):
            c = dict(base)
            c["z"] = np.array(base["z"])
            c["z"][[0, 7]] = bad
            got, ins, _ = run_core(core_exe, tmp_path, b, c, bits=bits)
            assert not ins[[0, 7]].any() and np.isnan(got[[0, 7]]).all()
            c["x"] = np.array(base["x"])
            c["x"][3] = bad
            assert not run_core(core_exe, tmp_path, b, c, bits=bits)[1][:, 3].any()
        for axis, n in (("r", 5), ("a", 4)):
            for i, v in ((1, None), (n - 1, None), (2, np.nan), (0, np.nan), (n - 1, np.inf)):
                c = dict(base)
                g = np.array(base[axis])
                g[i] = g[i - 1] if v is None else v                    # a repeated node; a NaN / Inf node
                c[axis] = g
                for bisect in (0, 1):
                    run_core(core_exe, tmp_path, b, c, bits=bits, bisect=bisect)
        c2 = R.polar_case("2x2")
        for bisect in (0, 1):
            run_core(core_exe, tmp_path, R.data((2, 2, 1), np.float64, 7), c2, bits=bits, bisect=bisect)
        # a uniform-looking axis whose interior is not: the guess is checked against the nodes
        c = dict(R.polar_case("64x33"))
        g = np.array(c["r"])
        g[1:-1] = g[0] + (g[-1] - g[0]) * np.linspace(0, 1, 64)[1:-1] ** 3
        c["r"] = g
        b64 = R.data((64, 33, 1), np.float64, 8)
        got, ins, flags = run_core(core_exe, tmp_path, b64, c, bits=bits)
        want, inside = _ref(b64, c)
        from tests.test_gpu_scanconvert import K
        real = np.float32 if bits == 32 else np.float64
        assert flags[0] == 0 and np.array_equal(ins, inside) and np.abs(got - want)[inside].max() <= bound(K[bits, "none"], real, c, b64, "none", -np.inf)


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_abi_symbol_and_descriptor_layout():
    L = _lib.lib()
    assert "qdas_scanconvert" in _lib.SYMBOLS and hasattr(L, "qdas_scanconvert")
    D = _lib.ScanconvertDesc
    assert C.sizeof(D) == 7 * 8 + 4 * 8 + 4 * 4 + 5 * 8 + 6 * 8 + 8
    assert (D.Z.offset, D.P.offset, D.sr.offset, D.dtype.offset, D.device.offset, D.origin.offset, D.fill.offset, D.r.offset, D.queue.offset) == (24, 48, 56, 88, 100, 104, 128, 144, 192)
    with open(os.path.join(ROOT, "include", "qdas.h")) as f:
        header = f.read()
    body = re.search(r"typedef struct qdas_scanconvert_desc \{(.*?)\} qdas_scanconvert_desc;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            rest = decl.split(None, 1 + decl.startswith("const"))[-1]
            names += [re.sub(r"\[\d+\]", "", n).strip(" *") for n in rest.split(",")]
    assert names == [n for n, _ in D._fields_]
    assert (_lib.SC_PRE_NONE, _lib.SC_PRE_ABS, _lib.SC_PRE_DB) == tuple(int(re.search(rf"#define QDAS_SC_PRE_{n}\s+(\d+)", header).group(1)) for n in ("NONE", "ABS", "DB"))
    import qups_amd
    for n in ("scan_convert", "scan_convert3"):
        assert n in qups_amd.__all__ and callable(getattr(qups_amd, n))


BUF = (C.c_double * 8)()
P = C.cast(BUF, C.c_void_p)


def _desc(**kw):
    d = _lib.ScanconvertDesc()
    d.R, d.A, d.E, d.Z, d.X, d.Y, d.P = 5, 4, 0, 7, 6, 0, 2
    d.sr, d.sa, d.se, d.sp = 1, 5, 0, 20
    d.dtype, d.cplx, d.pre, d.device = _lib.QDAS_F32, 1, _lib.SC_PRE_DB, -1
    d.fill, d.db_floor = math.nan, -math.inf
    d.r = d.a = d.e = d.x = d.y = d.z = P
    for k, v in kw.items():
        if k == "origin":
            d.origin[0], d.origin[1], d.origin[2] = v
        else:
            setattr(d, k, v)
    return d


@pytest.mark.parametrize("kw,code,text", [
    (dict(R=1), 1, "R = 1"), (dict(A=1), 1, "A = 1"), (dict(R=0), 1, "R = 0"), (dict(E=1), 1, "E is 0"),
    (dict(Y=3), 1, "Y must be 0"), (dict(E=3), 1, "Y >= 1"), (dict(dtype=2), 1, "dtype"), (dict(dtype=-1), 1, "dtype"),
    (dict(pre=3), 1, "pre"), (dict(pre=-1), 1, "pre"), (dict(cplx=2), 1, "cplx"), (dict(cplx=-1), 1, "cplx"),
    (dict(origin=(0.0, math.nan, 0.0)), 1, r"origin\[1\]"), (dict(origin=(math.inf, 0.0, 0.0)), 1, r"origin\[0\]"), (dict(origin=(0.0, 0.0, -math.inf)), 1, r"origin\[2\]"),
    (dict(db_floor=math.nan), 1, "db_floor"),
    (dict(r=None), 1, "null axis pointer"), (dict(a=None), 1, "null axis pointer"), (dict(x=None), 1, "null axis pointer"), (dict(z=None), 1, "null axis pointer"),
    (dict(E=2, Y=2, e=None), 1, "null axis pointer"), (dict(E=2, Y=2, y=None), 1, "null axis pointer"),
    (dict(R=8000, A=193), 2, "LDS"), (dict(R=4096, A=4095, E=2, Y=1), 2, "LDS"), (dict(R=1 << 40), 2, "LDS"),
    (dict(X=1 << 31), 2, "workgroups"), (dict(Z=1 << 40, X=1 << 10), 2, "workgroups"), (dict(E=2, Y=1 << 20, X=1 << 12), 2, "workgroups"),
    (dict(P=1 << 58), 2, "2\\^60"), (dict(sp=1 << 60), 2, "2\\^60"), (dict(sa=-(1 << 59)), 2, "2\\^60"), (dict(Z=1 << 30, X=1 << 29, P=4), 2, "2\\^60"),
])
def test_c_abi_rejects_bad_calls_before_any_launch(kw, code, text):
    """device = -1 and pointers to host memory: nothing here may reach a HIP call"""
    L = _lib.lib()
    assert L.qdas_scanconvert(C.byref(_desc(**kw)), P, P) == code
    assert re.search(text, L.qdas_last_error().decode()), L.qdas_last_error()


def test_c_abi_null_pointers_and_empty_problems():
    L = _lib.lib()
    assert L.qdas_scanconvert(None, P, P) == 1 and "null descriptor" in L.qdas_last_error().decode()
    for args, what in (((None, P), "b"), ((P, None), "out")):
        assert L.qdas_scanconvert(C.byref(_desc()), *args) == 1 and f"null data pointer ({what})" in L.qdas_last_error().decode()
    for kw in (dict(Z=0), dict(X=0), dict(P=0), dict(E=2, Y=2, Z=0)):
        assert L.qdas_scanconvert(C.byref(_desc(r=None, a=None, e=None, x=None, y=None, z=None, **kw)), None, None) == 0       # nothing to do, no device needed
    assert L.qdas_scanconvert(C.byref(_desc(Z=0, R=1)), None, None) == 1, "an empty call is still validated"
    assert L.qdas_scanconvert(C.byref(_desc(R=4096, A=4096)), None, P) == 1 and "null data" in L.qdas_last_error().decode()   # 64 KiB of float64 fit
    assert L.qdas_scanconvert(C.byref(_desc(fill=0.0, db_floor=-120.0, Z=0)), None, None) == 0


def test_the_stream_travels_in_the_descriptor_and_there_is_no_work_space():
    """the census of ``void *stream`` parameters (tests/test_streams_host.py) is a pinned list: the entry takes its stream in ``queue`` and its stream cases live
    in tests/test_gpu_scanconvert.py; the file constructs no Scratch (tests/test_scratch_host.py pins that list too), allocates and synchronises nothing"""
    with open(os.path.join(ROOT, "include", "qdas.h")) as f:
        header = f.read()
    assert not [n for n in stream_entries(header) if "scanconvert" in n]
    proto = re.search(r"\bqdas_scanconvert\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1)
    assert "stream" not in proto and "qdas_scanconvert_desc" in proto
    from tests import test_gpu_scanconvert as GS
    for name in GS.STREAM_CASES:
        assert name.startswith("test_") and callable(getattr(GS, name))
    from tests.test_scratch_host import scratch_users
    for fn in ("scanconvert.hip", "scanconvert_core.h"):
        with open(os.path.join(ROOT, "qups_amd", "csrc", fn)) as f:
            src = f.read()
        assert not scratch_users(src) and "hipMalloc" not in src and "Synchronize" not in src and "atomic" not in re.sub(r"//[^\n]*", "", src)
    with open(os.path.join(ROOT, "qups_amd", "csrc", "scanconvert_core.h")) as f:
        assert "hip/" not in f.read(), "the core has no HIP dependency"


# ---------------------------------------------------------------------------------------------------------------- the Python layer (no device)
def test_python_argument_handling():
    import torch
    cpu = torch.device("cpu")
    a = np.array([-37.0, 0.1, 12.5, 37.0])
    assert np.array_equal(SC.deg2rad(a), a * np.pi / 180) and SC.deg2rad([180.0])[0] == np.pi
    t = SC._axis(a, "a_deg", "scan_convert", cpu, True, angle=True)
    assert t.dtype == torch.float64 and np.array_equal(t.numpy(), R.deg2rad(a))
    assert np.array_equal(SC._axis(torch.from_numpy(a), "a_deg", "scan_convert", cpu, True, angle=True).numpy(), R.deg2rad(a))
    for g in ([0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [0.0, np.nan, 2.0], [0.0, np.inf]):
        with pytest.raises(DasError, match="the r axis must be finite and strictly increasing"):
            SC._axis(g, "r", "scan_convert", cpu, True)
        assert SC._axis(g, "r", "scan_convert", cpu, False).numel() == len(g), "check_grid=False: the caller's promise"
    for g in ([-180.0, 0.0], [0.0, 180.5], [-200.0, 300.0]):
        with pytest.raises(DasError, match=r"a_deg.*\(-180, 180\]"):
            SC._axis(g, "a_deg", "scan_convert", cpu, True, angle=True)
    assert SC._axis([-179.9, 180.0], "a_deg", "scan_convert", cpu, True, angle=True)[-1].item() == np.pi
    with pytest.raises(DasError, match="the a_deg axis needs at least 2 nodes"):
        SC._axis([1.0], "a_deg", "scan_convert", cpu, True, angle=True)
    assert SC._axis([1.0], "y", "scan_convert3", cpu, True, least=1).numel() == 1
    # pages: column-major trailing dimensions collapse, a row-major pair does not, size-1 dimensions do not count
    assert SC.page_stride((), ()) == (1, 0) and SC.page_stride((3,), (40,)) == (3, 40) and SC.page_stride((1, 3), (7, 40)) == (3, 40)
    assert SC.page_stride((2, 3), (20, 40)) == (6, 20) and SC.page_stride((2, 3), (60, 20)) == (6, None) and SC.page_stride((2, 3), (20, 50)) == (6, None)
    assert SC.page_stride((0, 3), (20, 40)) == (0, 0)
    das_view = torch.empty((3, 2, 1, 4, 5)).permute(4, 3, 2, 1, 0)                  # what DAS returns: I1 fastest
    assert SC.page_stride(das_view.shape[2:], das_view.stride()[2:]) == (6, 20)
    row_major = torch.empty((5, 4, 2, 3))
    assert SC.page_stride(row_major.shape[2:], row_major.stride()[2:]) == (6, None)
    assert SC.page_stride(row_major[..., 0].shape[2:], row_major[..., 0].stride()[2:]) == (2, 3)
    # refusals that need no device
    b = torch.zeros((5, 4))
    with pytest.raises(DasError, match="device tensor"):
        SC.scan_convert(b, np.arange(1.0, 6.0), a)
    with pytest.raises(DasError, match="device tensor"):
        SC.scan_convert3(torch.zeros((5, 4, 2)), np.arange(1.0, 6.0), a, [0.0, 1.0])
    with pytest.raises(DasError, match="Data must be in order 'RAY'"):
        Scan(G.scan_polar(np.arange(1.0, 6.0), a)).scanConvert(b)
    with pytest.raises(DasError, match="Data must be in order 'RAY'"):
        Scan.cartesian([0.0, 1.0], [0.0, 1.0]).scanConvert(b)
    with pytest.raises(DasError, match="scanC"):
        Scan.polar(np.arange(1.0, 6.0), a).scanConvert(b, Scan(G.scan_cartesian([0.0, 1.0], [0.0, 1.0])))
    with pytest.raises(DasError, match="device tensor"):
        Scan.polar(np.arange(1.0, 6.0), a).scanConvert(b)
    assert set(SC.PRE) == {"none", "abs", "db"}
