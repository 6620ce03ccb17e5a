"""The 'fdtd3' command of mex/qdas_mex.c, driven over the fake MEX runtime (tests/fake_mex/) and the real libqdas.so by tests/fake_mex/run_fdtd3.c, which
compares the result bit for bit with the C ABI called directly and writes it to a file; here the same case -- grid (a) of the parity list, three pulses --
goes through the Python layer (``qups_amd.fdtd3.fdtd3``) and must give the same bits."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_mex")
SRC = os.path.join(ROOT, "mex", "qdas_mex.c")
CFLAGS = ["-std=c99", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-I", os.path.join(ROOT, "include"), "-I", FAKE]


def build_gateway(tmp_path=None):
    import tempfile
    exe = os.path.join(str(tmp_path) if tmp_path is not None else tempfile.mkdtemp(prefix="qdas_mex_fdtd3_"), "run_fdtd3")
    lib = os.path.join(ROOT, "qups_amd")
    cmd = ["gcc", "-O1", *CFLAGS, SRC, os.path.join(FAKE, "fake_mex_runtime.c"), os.path.join(FAKE, "run_fdtd3.c"),
           "-L", lib, "-lqdas", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_gateway_and_fdtd3_driver_link(tmp_path):
    """without a device: the gateway, the fake runtime and the driver compile (-Wall -Wextra -Werror) and link against the library"""
    build_gateway(tmp_path)
    text = open(SRC).read()
    assert "'fdtd3'" in text and "qdas_fdtd3(" in text and "QDAS_FDTD3_ZERO" in text


def write_case(path, cs, R_, double):
    """the driver's input: the tables of ``qups_amd.fdtd3.prepare`` in the class under test"""
    from qups_amd import fdtd3 as F3
    rt = np.float64 if double else np.float32
    P = cs["P"]
    tab = F3.prepare(cs["c"], cs["rho"], cs["h"], cs["dt"], P)
    Nz, Nx, Ny = tab["Nz"], tab["Nx"], tab["Ny"]
    s = np.asarray(cs["s"], np.float64)
    Ts, M, V = s.shape
    node = lambda q: ((q[2] + P) * Nx + (q[1] + P)) * Nz + (q[0] + P)
    src_node, sen_node = node(cs["src"]), node(cs["sen"])
    csrc = tab["c"].reshape(-1)[src_node]
    w = [cs["nrm"][k] * 2.0 * csrc * cs["dt"] / cs["h"] for k in range(3)]           # (the Python layer's expression, term by term: the same float64 bits)
    with open(path, "wb") as f:
        np.array([int(double), Nz, Nx, Ny, V, cs["Nt"], M, Ts, len(sen_node), 2 * R_], np.int64).tofile(f)
        np.array([cs["dt"] / cs["h"], 1.0 / cs["h"]]).tofile(f)
        np.stack([tab[k] for k in ("c2", "rho", "dtrz", "dtrx", "dtry")]).astype(rt).tofile(f)
        np.concatenate([tab[k] for k in ("az", "azs", "ax", "axs", "ay", "ays")]).astype(rt).tofile(f)
        s.astype(rt).tofile(f)                                                       # T' x M x V in C order: pulse fastest, MATLAB's V x M x T'
        np.stack([src_node.astype(np.float64), *w], 1).tofile(f)
        sen_node.astype(np.float64).tofile(f)
    return len(sen_node), V


@pytest.mark.gpu
@pytest.mark.parametrize("double", [False, True], ids=["single", "double"])
def test_fdtd3_command_matches_the_c_abi_and_the_python_layer(tmp_path, double):
    from qups_amd import fdtd3 as F3
    from tests import fdtd3_ref as R3
    R_ = 4
    cs = R3.parity_case(*R3.GRIDS[0], 3)
    inp, dump = str(tmp_path / "case.bin"), str(tmp_path / "fdtd3.bin")
    N, V = write_case(inp, cs, R_, double)
    r = subprocess.run([build_gateway(tmp_path), inp, dump], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fdtd3 gateway OK" in r.stdout, r.stdout + r.stderr
    assert "bit-identical to the C ABI" in r.stdout
    rt = np.float64 if double else np.float32
    mex = np.fromfile(dump, rt).reshape(V, N, cs["Nt"]).transpose(2, 1, 0)           # MATLAB's Nt x N x V, time fastest in the file
    pos = lambda w: np.stack([cs["x"][cs[w][1]], cs["y"][cs[w][2]], cs["z"][cs[w][0]]])
    got = F3.fdtd3(cs["c"], cs["rho"], cs["z"], cs["x"], cs["y"], pos("src"), cs["nrm"], cs["s"], pos("sen"), cs["Nt"], cs["dt"], PML=cs["P"], order=2 * R_,
                   prec="double" if double else "single").cpu().numpy()
    assert got.shape == mex.shape and got.dtype == mex.dtype
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(mex).view(np.uint8))
