"""Straight-ray integrals without a GPU: the float64 restatement (tests/raypaths_ref.py) against the closed forms the contract implies; the walk the device
kernels compile (qups_amd/csrc/raypaths_walk.h) built for the host with the sanitizers and compared with the restatement; the Python layer's argument
handling; the C ABI's validation, which happens before any HIP call; the gateway's compile."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from qups_amd import DasError, _lib
from qups_amd import raypaths as RP
from tests import raypaths_ref as R
from tests.test_streams_host import stream_entries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = ["2x2", "11x9", "33x41", "2x65", "65x2"]
EPS = np.finfo(np.float64).eps


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in GRIDS:
        xg, zg = R.grids()[name]
        pa, pb = R.rays(xg, zg)
        out[name] = (xg, zg, pa, pb, R.dense_many(xg, zg, pa, pb))
    return out


@pytest.mark.parametrize("name", GRIDS)
def test_restatement_weight_sum_is_the_clipped_length_and_a_linear_field_is_exact(cases, name):
    """bounds: a ray has at most X + Z + 1 segments of 4 weights, each a handful of rounded operations on numbers of the size of the span: 64 eps of the
    longest ray is generous for the sums (the issue's figures: 3e-16 .. 9e-16).  The closed form subtracts, so a weight that should be 0 may come out as
    -1e-33: "no negative weight" is asserted to eps of the largest weight."""
    xg, zg, pa, pb, W = cases[name]
    J = pa.shape[1]
    L = np.array([R.clipped_length(xg, zg, pa[:, j], pb[:, j]) for j in range(J)])
    lin = (0.3, 1.7 / np.ptp(xg), -0.9 / np.ptp(zg))
    XX, ZZ = np.meshgrid(xg, zg, indexing="ij")
    I = np.array([R.linear_integral(xg, zg, pa[:, j], pb[:, j], *lin) for j in range(J)])
    assert np.abs(W.sum((1, 2)) - L).max() <= 64 * EPS * L.max()
    assert np.abs((W * (lin[0] + lin[1] * XX + lin[2] * ZZ)).sum((1, 2)) - I).max() <= 64 * EPS * np.abs(I).max()
    assert W.min() >= -EPS * W.max()
    assert (W[L == 0] == 0).all() and (L == 0).sum() >= 10


def test_restatement_on_the_32_sign_and_swap_cases():
    for xg, zg, a, b in R.sign_swap_cases():
        W = R.dense(xg, zg, a, b)
        assert abs(W.sum() - np.hypot(*(b - a))) <= 16 * EPS * 10 and W.min() >= 0
        assert np.abs(R.dense(xg, zg, b, a) - W).max() <= 16 * EPS
    assert len(R.sign_swap_cases()) == 32


def test_restatement_axis_aligned_rays_on_a_grid_line_weigh_only_that_line():
    xg, zg = R.grids()["33x41"]
    for i in (0, 7, 32):
        W = R.dense(xg, zg, (xg[i], zg[0]), (xg[i], zg[-1]))
        assert (np.delete(W, i, axis=0) == 0).all() and abs(W[i].sum() - np.ptp(zg)) <= 64 * EPS * np.ptp(zg)
    for k in (0, 20, 40):
        W = R.dense(xg, zg, (xg[-1], zg[k]), (xg[0], zg[k]))
        assert (np.delete(W, k, axis=1) == 0).all() and abs(W[:, k].sum() - np.ptp(xg)) <= 64 * EPS * np.ptp(xg)


def diagonal_weights(n_nodes, d, i0, k0, i1, k1):
    """closed form for a node-to-node diagonal on a square grid of pitch d.  Along a cell's diagonal u = v = t, so the hats of the two corners ON the diagonal
    are (1 - t)^2 and t^2 (mean 1/3 each) and those of the two corners OFF it are t (1 - t) (mean 1/6 each): per crossed cell, of length sqrt(2) d, the
    diagonal corners get sqrt(2) d / 3 and the off-diagonal corners sqrt(2) d / 6.  An interior node of the diagonal lies in two crossed cells (2/3 sqrt(2) d),
    an end node in one (half that).  (The feature's issue gave sqrt(2) d, half at the ends and nothing off the diagonal -- "the hats are linear along a cell's
    diagonal and vanish at its off-diagonal corners".  They are quadratic there: t (1 - t) is not 0, and the issue's own identity sum(w f) = the integral of
    the bilinear interpolant of f contradicts that figure for f = the hat of an off-diagonal corner.  Its figures do sum to the ray's length, as these do.)"""
    want = np.zeros((n_nodes, n_nodes))
    si, sk = np.sign(i1 - i0), np.sign(k1 - k0)
    seg = np.sqrt(2) * d
    for s in range(abs(i1 - i0)):
        i, k = i0 + s * si, k0 + s * sk
        want[i, k] += seg / 3
        want[i + si, k + sk] += seg / 3
        want[i + si, k] += seg / 6
        want[i, k + sk] += seg / 6
    return want


def test_restatement_node_to_node_diagonal_on_a_square_grid():
    d = 0.25
    g = d * np.arange(9.0)
    for i0, k0, i1, k1 in ((1, 1, 6, 6), (7, 2, 3, 6), (0, 8, 8, 0)):
        W = R.dense(g, g, (g[i0], g[k0]), (g[i1], g[k1]))
        want = diagonal_weights(9, d, i0, k0, i1, k1)
        n = abs(i1 - i0)
        assert np.abs(W - want).max() <= 16 * EPS
        assert abs(want[i0, k0] - np.sqrt(2) * d / 3) <= EPS and abs(want[i0 + np.sign(i1 - i0), k0 + np.sign(k1 - k0)] - 2 * np.sqrt(2) * d / 3) <= EPS
        assert np.count_nonzero(W) == (n + 1) + 2 * n and abs(W.sum() - n * np.sqrt(2) * d) <= 16 * EPS


# ---------------------------------------------------------------------------------------------------------------- the device's walk, on the host
@pytest.fixture(scope="module")
def walk_exe(tmp_path_factory):
    """raypaths_walk.h under AddressSanitizer and UBSan in a stand-alone program: the grid vectors are heap arrays of exactly X and Z values"""
    exe = str(tmp_path_factory.mktemp("walk") / "raypaths_walk_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=fast", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "qups_amd", "csrc"), os.path.join(ROOT, "tests", "raypaths_walk_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _walk(exe, tmp_path, bits, xg, zg, pa, pb):
    J = pa.shape[1]
    path = str(tmp_path / "rays.txt")
    with open(path, "w") as f:
        f.write(f"{bits} {xg.size} {zg.size} {J}\n" + " ".join(repr(float(v)) for v in xg) + "\n" + " ".join(repr(float(v)) for v in zg) + "\n")
        for j in range(J):
            f.write(" ".join(repr(float(v)) for v in (pa[0, j], pa[1, j], pb[0, j], pb[1, j])) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = [line.split() for line in r.stdout.strip().split("\n")]
    steps = np.array([[int(row[0]), int(row[1])] for row in rows])
    return np.array([[float(v) for v in row[2:]] for row in rows]).reshape(J, xg.size, zg.size), steps


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("name", GRIDS)
def test_the_walk_on_the_host_matches_the_restatement(cases, walk_exe, tmp_path, name, bits):
    """the program itself fails on a slot beyond K, an index outside the grid, a negative or non-finite weight, a sanitizer report; here the dense sums meet
    the restatement within the bounds of the device test (same text, same bounds), dead rays emit nothing and no ray needs more than X + Z - 1 steps"""
    from tests.test_gpu_raypaths import TOL
    import torch
    dtype = torch.float64 if bits == 64 else torch.float32
    xg, zg, pa, pb, W64 = cases[name]
    if bits == 32:
        xg, zg, pa, pb = (np.asarray(v, np.float32).astype(np.float64) for v in (xg, zg, pa, pb))
        W64 = R.dense_many(xg, zg, pa, pb)
    W, steps = _walk(walk_exe, tmp_path, bits, xg, zg, pa, pb)
    L = np.array([R.clipped_length(xg, zg, pa[:, j], pb[:, j]) for j in range(pa.shape[1])])
    ew, el = np.abs(W - W64).max() / W64.max(), np.abs(W.sum((1, 2)) - L).max() / L.max()
    print(f"host walk {name} f{bits}: dense {ew:.3e} length {el:.3e}, at most {steps[:, 0].max()} of {xg.size + zg.size + 1} slots")
    assert ew <= TOL["w", dtype] and el <= TOL["i", dtype]
    assert (steps[L == 0, 1] == 0).all() and steps[:, 0].max() <= xg.size + zg.size - 1


def test_the_walk_ends_on_a_broken_grid(walk_exe, tmp_path):
    """NaN, Inf, equal and decreasing grid values (the caller broke its promise): the walk still ends inside its K slots with indices inside the grid and
    no negative or non-finite weight -- the program checks that -- whatever the ray"""
    xg, zg = R.grids()["11x9"]
    pa, pb = R.rays(xg, zg)
    for bits in (64, 32):
        for bad in (np.nan, np.inf, -np.inf):
            for i in (0, 5, 10):
                x = xg.copy()
                x[i] = bad
                _walk(walk_exe, tmp_path, bits, x, zg, pa, pb)
            z = zg.copy()
            z[[2, 8]] = bad
            _walk(walk_exe, tmp_path, bits, xg, z, pa, pb)
        _walk(walk_exe, tmp_path, bits, xg[::-1].copy(), zg, pa, pb)
        _walk(walk_exe, tmp_path, bits, np.zeros(11), np.repeat(zg[:3], 3), pa, pb)


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_abi_symbols_and_descriptor():
    L = _lib.lib()
    for s in ("qdas_raypaths_slots", "qdas_raypaths_weights", "qdas_raypaths_integrate"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
    D = _lib.RaypathsDesc
    assert C.sizeof(D) == 112                                            # 4 extents, 4 strides, 2 ints, 5 pointers
    assert (D.F.offset, D.xstride.offset, D.pb_stride.offset, D.dtype.offset, D.device.offset, D.xg.offset, D.pb.offset, D.queue.offset) == (24, 32, 56, 64, 68, 72, 96, 104)
    with open(os.path.join(ROOT, "include", "qdas.h")) as f:
        header = f.read()
    body = re.search(r"typedef struct qdas_raypaths_desc \{(.*?)\} qdas_raypaths_desc;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1 + decl.strip().startswith("const"))[-1].split(",")]
    assert names == [n for n, _ in D._fields_]
    assert L.qdas_version() == 103 and L.qdas_raypaths_slots(512, 512) == 1025
    import qups_amd
    for n in ("wbilerpg", "ray_integrals", "rayPaths", "globalAverageC"):
        assert n in qups_amd.__all__ and callable(getattr(qups_amd, n))


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
])
def test_c_abi_rejects_bad_calls_before_any_launch(kw, code, text):
    """device = -1 and pointers to host memory: nothing here may reach a HIP call"""
    L = _lib.lib()
    for call in (lambda d: L.qdas_raypaths_weights(C.byref(d), P, P, P), lambda d: L.qdas_raypaths_integrate(C.byref(d), P, P, P)):
        assert call(_desc(**kw)) == code
        assert re.search(text, L.qdas_last_error().decode())


def test_c_abi_null_outputs_empty_problems_and_limits():
    L = _lib.lib()
    assert L.qdas_raypaths_weights(None, P, P, P) == 1 and L.qdas_raypaths_integrate(None, P, P, P) == 1
    for args in ((None, P, P), (P, None, P), (P, P, None)):
        assert L.qdas_raypaths_weights(C.byref(_desc()), *args) == 1 and "null data pointer" in L.qdas_last_error().decode()
    for args in ((None, P, P), (P, None, P)):
        assert L.qdas_raypaths_integrate(C.byref(_desc()), *args) == 1 and "null data pointer" in L.qdas_last_error().decode()
    assert L.qdas_raypaths_weights(C.byref(_desc(J=0, xg=None, zg=None, pa=None, pb=None)), None, None, None) == 0          # nothing to do, no device needed
    for kw in (dict(J=0), dict(F=0)):
        assert L.qdas_raypaths_integrate(C.byref(_desc(xg=None, zg=None, pa=None, pb=None, **kw)), None, None, None) == 0
    assert L.qdas_raypaths_integrate(C.byref(_desc(F=65536)), P, P, P) == 2 and "65535" in L.qdas_last_error().decode()
    assert L.qdas_raypaths_integrate(C.byref(_desc(zstride=1 << 61)), P, P, P) == 2
    assert L.qdas_raypaths_weights(C.byref(_desc(X=4096, Z=4096)), None, P, P) == 1                                         # 64 KiB of doubles fit


def test_the_stream_travels_in_the_descriptor_and_has_its_case_in_the_gpu_file():
    """the census of ``void *stream`` parameters (tests/test_streams_host.py) is a pinned list: the entries take their stream in ``queue``, their stream case
    lives in tests/test_gpu_raypaths.py; and the file constructs no Scratch (tests/test_scratch_host.py pins that list too): there is no work space"""
    with open(os.path.join(ROOT, "include", "qdas.h")) as f:
        header = f.read()
    assert not [n for n in stream_entries(header) if "raypaths" in n]
    for name in ("qdas_raypaths_weights", "qdas_raypaths_integrate"):
        proto = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1)
        assert "stream" not in proto and "qdas_raypaths_desc" in proto
    from tests import test_gpu_raypaths as G
    for name in G.STREAM_CASES:
        assert name.startswith("test_") and callable(getattr(G, name))
    from tests.test_scratch_host import scratch_users
    for fn in ("raypaths.hip", "raypaths_walk.h"):
        with open(os.path.join(ROOT, "qups_amd", "csrc", fn)) as f:
            src = f.read()
        assert not scratch_users(src) and "hipMalloc" not in src and "Synchronize" not in src


# ---------------------------------------------------------------------------------------------------------------- the Python layer (no device)
def test_python_helpers_and_refusals():
    import torch
    assert RP.slots(512, 512) == 1025 and RP.default_bsize(11, 9, 1) == (1 << 32) // (21 * 128) and RP.default_bsize(5000, 5000, 1 << 20) == 1
    assert RP._strides("ZX", 11, 9) == (9, 1) and RP._strides("XZ", 11, 9) == (1, 11)
    with pytest.raises(DasError, match="ord"):
        RP._strides("YX", 2, 2)
    assert RP._dtype_of(np.zeros(2, np.float32), torch.zeros(2)) == torch.float32
    assert RP._dtype_of(np.zeros(2, np.float32), np.zeros(2)) == torch.float64 and RP._dtype_of([0, 1]) == torch.float64
    for bad in (torch.zeros(2, dtype=torch.float16), np.zeros(2, np.float16), np.zeros(2, np.complex64)):
        with pytest.raises(DasError):
            RP._dtype_of(bad)
    cpu = torch.device("cpu")
    for g in ([0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [0.0, np.nan, 2.0], [0.0, np.inf]):
        with pytest.raises(DasError, match="monotonic"):
            RP._grid(g, "x", torch.float64, cpu, True)
    with pytest.raises(DasError, match="at least 2"):
        RP._grid([1.0], "z", torch.float64, cpu, True)
    assert RP._grid(np.arange(4.0), "x", torch.float32, cpu, True).dtype == torch.float32
    a, b, J, sa, sb = RP._pair([0.0, 1.0], np.zeros((2, 7)), torch.float64, cpu)
    assert (J, sa, sb) == (7, 0, 1) and tuple(a.shape) == (1, 2) and tuple(b.shape) == (7, 2) and b.is_contiguous()
    assert RP._pair(np.zeros((2, 7)), np.zeros((2, 1)), torch.float64, cpu)[2:] == (7, 1, 0)
    assert RP._pair(np.zeros((2, 1)), np.zeros((2, 1)), torch.float64, cpu)[2:] == (1, 1, 1)
    with pytest.raises(DasError, match="equal counts"):
        RP._pair(np.zeros((2, 3)), np.zeros((2, 7)), torch.float64, cpu)
    with pytest.raises(DasError, match="2 x J"):
        RP._points(np.zeros((3, 4)), "pa", torch.float64, cpu)
    with pytest.raises(NotImplementedError, match="xiaolin"):
        RP.rayPaths([0.0, 1.0], [0.0, 1.0], np.zeros((2, 1)), np.zeros((2, 1)), method="xiaolin")
    with pytest.raises(DasError, match="device tensor"):
        RP.ray_integrals(torch.zeros(2, 2), [0.0, 1.0], [0.0, 1.0], [0, 0], [1, 1])
    with pytest.raises(DasError, match="device tensor"):
        RP.globalAverageC(torch.ones(2, 2), [0.0, 1.0], [0.0, 1.0], [0, 0], [[1], [1]])
    with pytest.raises(DasError, match="ord"):
        RP.ray_integrals(torch.zeros(2, 2), [0.0, 1.0], [0.0, 1.0], [0, 0], [1, 1], ord="xz")


# ---------------------------------------------------------------------------------------------------------------- the gateway
def test_gateway_and_raypaths_driver_compile(tmp_path):
    fake = os.path.join(ROOT, "tests", "fake_mex")
    cflags = ["-std=c99", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-I", os.path.join(ROOT, "include"), "-I", fake]
    src = os.path.join(ROOT, "mex", "qdas_mex.c")
    for s in (src, os.path.join(fake, "run_raypaths.c")):
        r = subprocess.run(["gcc", "-c", *cflags, s, "-o", str(tmp_path / (os.path.basename(s) + ".o"))], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    text = open(src).read()
    assert "'wbilerp'" in text and "'rayintegrals'" in text and "qdas_raypaths_weights(" in text and "qdas_raypaths_integrate(" in text
