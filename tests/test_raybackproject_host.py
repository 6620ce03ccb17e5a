"""The transposed straight-ray product without a GPU: the weight one ray gives one node (qups_amd/csrc/raypaths_node.h, the text the back-projection kernel
compiles) built for the host with the sanitizers into a stand-alone program and compared with the float64 restatement (tests/raypaths_ref.py); the adjoint
identity between the two; qdas_raypaths_backproject's validation, which happens before any HIP call; the census facts; the kernels' register metadata; the
Python layer's refusals; SART on the restatement's matrix (tests/raysart_ref.py).

TOLERANCES of the per-node weights, max |host - ref| / max |ref| over the five grids of raypaths_ref.grids() with raypaths_ref.rays() and the 32 sign / swap
cases, as tests/raypaths_node_host.cpp itself gives them (for float32 the restatement gets the float32-rounded grid and points):
    float64   7.3e-15 (the 33 x 41 millimetre grid) -> 3e-14       cap 4e-14, the forward walk's test constant: the same numbers, no reason to be worse
    float32   2.8e-6  (33 x 41, 65 x 2)             -> 2e-5        cap 2e-5, the forward's
Each constant is 4 x the measured figure rounded up to one digit."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from qups_amd import DasError, _lib
from qups_amd import raypaths as RP
from tests import raypaths_ref as R
from tests import raysart_ref as S
from tests.test_streams_host import stream_entries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = ["2x2", "11x9", "9x11", "33x41", "2x65", "65x2"]
NODE_MEASURED = {64: 7.3e-15, 32: 2.8e-6}
NODE_TOL = {64: 3e-14, 32: 2e-5}
NODE_CAP = {64: 4e-14, 32: 2e-5}


def rays_of(name, bits):
    """grid and rays of one case (11x9 and 9x11 carry the reference's 32 sign / swap cases), rounded to the data's precision, and the restatement's weights"""
    if name == "9x11":
        cs = R.sign_swap_cases()[16:]
        xg, zg = cs[0][0], cs[0][1]
        pa, pb = np.stack([c[2] for c in cs], 1), np.stack([c[3] for c in cs], 1)
    else:
        xg, zg = R.grids()[name]
        pa, pb = R.rays(xg, zg)
        if name == "11x9":
            cs = R.sign_swap_cases()[:16]
            pa, pb = np.concatenate([pa, np.stack([c[2] for c in cs], 1)], 1), np.concatenate([pb, np.stack([c[3] for c in cs], 1)], 1)
    if bits == 32:
        xg, zg, pa, pb = (np.asarray(v, np.float32).astype(np.float64) for v in (xg, zg, pa, pb))
    return xg, zg, pa, pb


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in GRIDS:
        for bits in (64, 32):
            xg, zg, pa, pb = rays_of(name, bits)
            out[name, bits] = (xg, zg, pa, pb, R.dense_many(xg, zg, pa, pb))
    return out


# ---------------------------------------------------------------------------------------------------------------- the per-node weight, on the host
@pytest.fixture(scope="module")
def node_exe(tmp_path_factory):
    """raypaths_node.h under AddressSanitizer and UBSan in a stand-alone program: the grid vectors are heap arrays of exactly X and Z values"""
    exe = str(tmp_path_factory.mktemp("node") / "raypaths_node_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=fast", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "qups_amd", "csrc"), os.path.join(ROOT, "tests", "raypaths_node_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _nodes(exe, tmp_path, bits, xg, zg, pa, pb):
    """``(W, hit)``: ``J x X x Z`` per-node weights and the number of 8 x 8 tiles whose slab test each ray passes"""
    J = pa.shape[1]
    path = str(tmp_path / "rays.txt")
    with open(path, "w") as f:
        f.write(f"{bits} {xg.size} {zg.size} {J}\n" + " ".join(repr(float(v)) for v in xg) + "\n" + " ".join(repr(float(v)) for v in zg) + "\n")
        for j in range(J):
            f.write(" ".join(repr(float(v)) for v in (pa[0, j], pa[1, j], pb[0, j], pb[1, j])) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = [line.split() for line in r.stdout.strip().split("\n")]
    return np.array([[float(v) for v in row[1:]] for row in rows]).reshape(J, xg.size, zg.size), np.array([int(row[0]) for row in rows])


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("name", GRIDS)
def test_the_node_weights_on_the_host_match_the_restatement(cases, node_exe, tmp_path, name, bits):
    """the program itself fails on a negative or non-finite weight, on a weight in a tile whose slab test the ray missed and on a sanitizer report; here the
    weights meet the restatement, a ray that gives nothing in the forward entries gives nothing, and what the restatement leaves at 0 is 0 exactly (grid-line
    rays weigh their line only)"""
    xg, zg, pa, pb, W64 = cases[name, bits]
    W, hit = _nodes(node_exe, tmp_path, bits, xg, zg, pa, pb)
    L = np.array([R.clipped_length(xg, zg, pa[:, j], pb[:, j]) for j in range(pa.shape[1])])
    ew, el = np.abs(W - W64).max() / W64.max(), np.abs(W.sum((1, 2)) - L).max() / L.max()
    print(f"host node weights {name} f{bits}: dense {ew:.3e} length {el:.3e}")
    assert NODE_TOL[bits] <= NODE_CAP[bits] and NODE_TOL[bits] >= 4 * NODE_MEASURED[bits]
    assert ew <= NODE_TOL[bits] and el <= NODE_TOL[bits]
    assert (W[L == 0] == 0).all() and (hit[L > 0] > 0).all()
    assert (W[W64 == 0] == 0).all()


def test_the_node_weights_stay_finite_and_non_negative_on_a_broken_grid(node_exe, tmp_path):
    """NaN, Inf, equal and decreasing grid values (the caller broke its promise), the grids the walk's host test uses: the program checks every weight"""
    xg, zg = R.grids()["11x9"]
    pa, pb = R.rays(xg, zg)
    for bits in (64, 32):
        for bad in (np.nan, np.inf, -np.inf):
            for i in (0, 5, 10):
                x = xg.copy()
                x[i] = bad
                _nodes(node_exe, tmp_path, bits, x, zg, pa, pb)
            z = zg.copy()
            z[[2, 8]] = bad
            _nodes(node_exe, tmp_path, bits, xg, z, pa, pb)
        _nodes(node_exe, tmp_path, bits, xg[::-1].copy(), zg, pa, pb)
        _nodes(node_exe, tmp_path, bits, np.zeros(11), np.repeat(zg[:3], 3), pa, pb)


@pytest.mark.parametrize("name", ["11x9", "33x41"])
def test_the_transposed_restatement_against_the_per_node_sums_and_the_adjoint_identity(cases, node_exe, tmp_path, name):
    """g = sum_j w_j r[j] from the per-node weights against the restatement's A' r, and <A s, r> = <s, A' r> with A the restatement and A' the per-node
    sums.  Bound: each weight is within NODE_TOL of the largest, so a sum of weights times values differs by at most that times the sum of |values| over
    the entries either matrix holds."""
    xg, zg, pa, pb, W64 = cases[name, 64]
    W, _ = _nodes(node_exe, tmp_path, 64, xg, zg, pa, pb)
    rng = np.random.default_rng(21)
    r, s = rng.standard_normal(W.shape[0]), rng.standard_normal(W.shape[1:])
    held = (W > 0) | (W64 != 0)                                  # (the restatement subtracts: a weight that should be 0 may come out as -1e-33)
    g, g64 = np.einsum("jxz,j->xz", W, r), np.einsum("jxz,j->xz", W64, r)
    assert (np.abs(g - g64) <= NODE_TOL[64] * W64.max() * np.einsum("jxz,j->xz", held, np.abs(r))).all()
    lhs, rhs = np.dot(np.einsum("jxz,xz->j", W64, s), r), np.sum(s * g)
    assert abs(lhs - rhs) <= NODE_TOL[64] * W64.max() * np.einsum("jxz,j,xz->", held, np.abs(r), np.abs(s))
    assert abs(np.dot(np.einsum("jxz,xz->j", W64, s), r) - np.sum(s * g64)) <= 64 * np.finfo(np.float64).eps * np.einsum("jxz,j,xz->", W64, np.abs(r), np.abs(s))


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_abi_symbol_argtypes_and_version():
    L = _lib.lib()
    assert "qdas_raypaths_backproject" in _lib.SYMBOLS and hasattr(L, "qdas_raypaths_backproject")
    assert L.qdas_raypaths_backproject.argtypes == [C.POINTER(_lib.RaypathsDesc), C.c_void_p, C.c_void_p, C.c_void_p]
    assert L.qdas_version() == 103 and C.sizeof(_lib.RaypathsDesc) == 112
    import qups_amd
    for n in ("ray_backproject", "ray_sart"):
        assert n in qups_amd.__all__ and n in RP.__all__ and callable(getattr(qups_amd, n))


BUF = (C.c_double * 8)()
P = C.cast(BUF, C.c_void_p)


def _desc(**kw):
    d = _lib.RaypathsDesc()
    d.X, d.Z, d.J, d.F = 11, 9, 5, 1
    d.xstride, d.zstride, d.pa_stride, d.pb_stride = 9, 1, 1, 1
    d.dtype, d.device = _lib.QDAS_F64, -1
    d.xg = d.zg = d.pa = d.pb = P
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("kw,code,text", [
    (dict(X=1), 1, "2 x 2"), (dict(Z=1), 1, "2 x 2"), (dict(X=0), 1, "2 x 2"), (dict(dtype=2), 1, "double or single"),
    (dict(pa_stride=2), 1, "0 or 1"), (dict(pb_stride=-1), 1, "0 or 1"),
    (dict(xg=None), 1, "null data pointer"), (dict(zg=None), 1, "null data pointer"), (dict(pa=None), 1, "null data pointer"), (dict(pb=None), 1, "null data pointer"),
    (dict(X=1 << 31), 2, "nodes per axis"), (dict(X=8000, Z=193), 2, "LDS"), (dict(X=16000, Z=385, dtype=1), 2, "LDS"), (dict(J=1 << 40), 2, "workgroups"),
    (dict(F=65536), 2, "65535"), (dict(zstride=1 << 61), 2, "2\\^60"), (dict(xstride=-(1 << 61)), 2, "2\\^60"),
])
def test_c_abi_rejects_bad_calls_before_any_launch(kw, code, text):
    """device = -1 and pointers to host memory: nothing here may reach a HIP call.  The rows of the forward entries (the same grids are taken both ways) and
    the ones of this entry; every text names the entry"""
    L = _lib.lib()
    assert L.qdas_raypaths_backproject(C.byref(_desc(**kw)), P, P, P) == code
    msg = L.qdas_last_error().decode()
    assert re.search(text, msg) and msg.startswith("raypaths_backproject:")


def test_c_abi_null_outputs_empty_problems_and_the_rule_for_no_vectors():
    L = _lib.lib()
    assert L.qdas_raypaths_backproject(None, P, P, P) == 1 and "null descriptor" in L.qdas_last_error().decode()
    for args in ((None, P, P), (P, None, P), (None, None, P)):                                # r and g are needed while F > 0
        assert L.qdas_raypaths_backproject(C.byref(_desc()), *args) == 1 and "null data pointer" in L.qdas_last_error().decode()
    # F = 0: a non-NULL colsum is the whole job -- without one there is nothing to write, and nothing is looked at
    assert L.qdas_raypaths_backproject(C.byref(_desc(F=0, xg=None, zg=None, pa=None, pb=None)), None, None, None) == 0
    assert L.qdas_raypaths_backproject(C.byref(_desc(F=0, J=0, xg=None, zg=None, pa=None, pb=None)), None, None, None) == 0
    # ... with one the grid is needed (r and g are not): the null row still fires before any HIP call
    assert L.qdas_raypaths_backproject(C.byref(_desc(F=0, xg=None)), None, None, P) == 1 and "null data pointer" in L.qdas_last_error().decode()
    assert L.qdas_raypaths_backproject(C.byref(_desc(F=0, pa=None)), None, None, P) == 1
    # J = 0 writes zeros: the maps are needed, the points and r are not -- but the grid vectors are read
    assert L.qdas_raypaths_backproject(C.byref(_desc(J=0)), None, None, None) == 1 and "null data pointer" in L.qdas_last_error().decode()
    assert L.qdas_raypaths_backproject(C.byref(_desc(J=0, zg=None)), None, P, None) == 1


def test_the_header_says_which_rule_for_no_vectors_and_no_rays():
    with open(os.path.join(ROOT, "include", "qdas.h")) as f:
        header = f.read()
    doc = header[header.index("The transposed product"):header.index("int qdas_raypaths_backproject")]
    assert "F = 0: a non-NULL colsum is the whole job" in doc and "J = 0 writes zeros" in doc


def test_census_no_stream_parameter_no_work_space_no_synchronisation_no_atomics():
    """the census of ``void *stream`` parameters and the list of Scratch users are pinned lists in existing tests: the entry takes its stream in ``queue`` and
    has no work space; its stream case lives in tests/test_gpu_raybackproject.py"""
    with open(os.path.join(ROOT, "include", "qdas.h")) as f:
        header = f.read()
    assert not [n for n in stream_entries(header) if "raypaths" in n]
    proto = re.search(r"\bqdas_raypaths_backproject\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1)
    assert "stream" not in proto and "qdas_raypaths_desc" in proto
    from tests.test_scratch_host import scratch_users
    for fn in ("raypaths.hip", "raypaths_walk.h", "raypaths_node.h"):
        with open(os.path.join(ROOT, "qups_amd", "csrc", fn)) as f:
            src = f.read()
        assert not scratch_users(src) and "hipMalloc" not in src and "Synchronize" not in src
        assert not re.search(r"atomic[A-Z_]|__hip_atomic|__atomic", src), fn
    with open(os.path.join(ROOT, "tests", "test_gpu_raybackproject.py")) as f:
        gpu = f.read()
    names = re.search(r"^STREAM_CASES = \((.*?)\)$", gpu, flags=re.M).group(1)
    for name in re.findall(r'"(\w+)"', names):
        assert name.startswith("test_") and re.search(r"^def " + name + r"\(", gpu, flags=re.M)
    assert re.findall(r'"(\w+)"', names)


def test_the_kernels_use_no_scratch_no_lds_and_spill_nothing():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    so = os.path.join(ROOT, "qups_amd", "libqdas.so")
    assert os.path.exists(kernel_regs.READELF), "llvm-readelf is part of the toolchain that built the library"
    rows = kernel_regs.kernel_table(so)
    names = kernel_regs.demangle([r["name"] for r in rows])
    mine = [(n, r) for n, r in zip(names, rows) if "backproject_kernel" in n]
    assert sorted(re.search(r"<(\w+)>", n).group(1) for n, _ in mine) == ["double", "float"]
    for n, r in mine:
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r["lds"] == 0, (n, r)
        assert r["vgpr"] + r["agpr"] <= 128, (n, r)                          # four waves per SIMD: the four tiles of a workgroup and three more groups


# ---------------------------------------------------------------------------------------------------------------- the Python layer (no device)
def test_python_refusals():
    import torch
    x, z = [0.0, 1.0], [0.0, 1.0]
    for bad in (torch.zeros(3, dtype=torch.float16), torch.zeros(3, dtype=torch.bfloat16)):
        with pytest.raises(DasError, match="half precision"):
            RP.ray_backproject(bad, x, z, [0, 0], [1, 1])
    with pytest.raises(DasError, match="real data"):
        RP.ray_backproject(torch.zeros(3, dtype=torch.complex64), x, z, [0, 0], [1, 1])
    with pytest.raises(DasError, match="float32 or float64"):
        RP.ray_backproject(torch.zeros(3, dtype=torch.int32), x, z, [0, 0], [1, 1])
    for shape in ((), (2, 3, 4)):
        with pytest.raises(DasError, match="F x J"):
            RP.ray_backproject(torch.zeros(shape), x, z, [0, 0], [1, 1])
    with pytest.raises(DasError, match="device tensor"):
        RP.ray_backproject(torch.zeros(3), x, z, [0, 0], [1, 1])
    with pytest.raises(DasError, match="device tensor"):
        RP.ray_backproject(np.zeros(3), x, z, [0, 0], [1, 1])
    with pytest.raises(DasError, match="ord"):
        RP.ray_backproject(torch.zeros(3), x, z, [0, 0], [1, 1], ord="zx")
    s0 = torch.zeros(2, 2)
    for relax in (0, 2, -0.5, 2.5, float("nan")):
        with pytest.raises(DasError, match="relax"):
            RP.ray_sart(torch.zeros(1), x, z, [0, 0], [1, 1], s0, relax=relax)
    for iters in (-1, 1.5, True):
        with pytest.raises(DasError, match="iters"):
            RP.ray_sart(torch.zeros(1), x, z, [0, 0], [1, 1], s0, iters=iters)
    with pytest.raises(DasError, match="half precision"):
        RP.ray_sart(torch.zeros(1), x, z, [0, 0], [1, 1], s0.half())
    with pytest.raises(DasError, match="device tensor"):
        RP.ray_sart(torch.zeros(1), x, z, [0, 0], [1, 1], s0)
    with pytest.raises(DasError, match="ord"):
        RP.ray_sart(torch.zeros(1), x, z, [0, 0], [1, 1], s0, ord="YX")


# ---------------------------------------------------------------------------------------------------------------- SART on the restatement
@pytest.mark.parametrize("name", ["11x9", "33x41"])
def test_sart_on_the_restatement_never_raises_the_weighted_residual(name):
    """16 x 16 top-to-bottom and 8 x 8 left-to-right edge rays through a Gaussian inclusion of +60 m/s in 1540, relax = 1, 30 steps from the homogeneous map:
    the R-weighted residual sqrt(sum (t - A s)^2 / len) does not increase (SART descends on it for relax in (0, 2)); no ray and no node is empty.  Recovery of
    the inclusion is NOT asserted: 320 rays do not determine 1353 nodes."""
    c = S.case(name)
    A = c["A"]
    assert A.shape == (320, c["X"] * c["Z"]) and (A.sum(1) > 0).all() and (A.sum(0) > 0).all()
    maps, res = S.sart(A, c["t"], c["s0"], 30)
    print(f"SART on the restatement {name}: weighted residual {res[0]:.3e} -> {res[-1]:.3e}")
    assert len(res) == 31 and all(b <= a for a, b in zip(res, res[1:])) and res[-1] < 0.1 * res[0]
    assert np.isfinite(maps[-1]).all()
