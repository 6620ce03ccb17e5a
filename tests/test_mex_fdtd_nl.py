"""The 'fdtdnl' command of mex/qdas_mex.c, driven over the fake MEX runtime (tests/fake_mex/) and the real libqdas.so by tests/fake_mex/run_fdtd_nl.c, which
compares the result bit for bit with the C ABI (``qdas_fdtd_nonlinear``) called directly and writes it to a file; here the same case -- the (37, 29, 6) grid
of the parity list driven hard (``tests/fdtd_nl_ref.nl_case``), three pulses, with and without the loss block of ``tests/fdtd_loss_ref.loss_case`` -- goes
through the Python layer (``qups_amd.fdtd.fdtd(BoA=...)``) and must give the same bits."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_mex_fdtd import CFLAGS, FAKE, ROOT, SRC


def build_gateway(tmp_path=None):
    import tempfile
    exe = os.path.join(str(tmp_path) if tmp_path is not None else tempfile.mkdtemp(prefix="qdas_mex_fdtd_nl_"), "run_fdtd_nl")
    lib = os.path.join(ROOT, "qups_amd")
    cmd = ["gcc", "-O1", *CFLAGS, SRC, os.path.join(FAKE, "fake_mex_runtime.c"), os.path.join(FAKE, "run_fdtd_nl.c"),
           "-L", lib, "-lqdas", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_gateway_and_fdtdnl_driver_link(tmp_path):
    """without a device: the gateway, the fake runtime and the driver compile (-Wall -Wextra -Werror) and link against the library"""
    build_gateway(tmp_path)
    text = open(SRC).read()
    assert "'fdtdnl'" in text and "qdas_fdtd_nonlinear(" in text and '"fdtdnl"' in text


def write_case(path, cs, ls, R_, double, convective):
    """the driver's input: the tables of ``qups_amd.fdtd.prepare``, the extended loss map and the extended map bq in the class under test"""
    from qups_amd import _lib
    from qups_amd import fdtd as F
    rt = np.float64 if double else np.float32
    P = cs["P"]
    tab = F.prepare(cs["c"], cs["rho"], cs["h"], cs["dt"], P)
    Nz, Nx = tab["Nz"], tab["Nx"]
    s = np.asarray(cs["s"], np.float64)
    Ts, M, V = s.shape
    src_node = (cs["src"][1] + P) * Nz + cs["src"][0] + P
    sen_node = (cs["sen"][1] + P) * Nz + cs["sen"][0] + P
    csrc = tab["c"].reshape(-1)[src_node]
    wz, wx = (cs["nrm"][k] * 2.0 * csrc * cs["dt"] / cs["h"] for k in (0, 1))        # (the Python layer's expression, term by term: the same float64 bits)
    L = 0 if ls is None else len(ls["g"])
    ext = lambda m: np.ascontiguousarray(np.pad(m, P, mode="edge").T).astype(rt)
    with open(path, "wb") as f:
        np.array([int(double), Nz, Nx, V, cs["Nt"], M, Ts, len(sen_node), 2 * R_, L, 0 if ls is None else 1, 0 if convective else _lib.FDTD_NL_NO_CONVECTIVE],
                 np.int64).tofile(f)
        np.array([cs["dt"] / cs["h"], 1.0 / cs["h"]]).tofile(f)
        np.stack([tab[k] for k in ("c2", "rho", "dtrz", "dtrx")]).astype(rt).tofile(f)
        np.concatenate([tab[k] for k in ("az", "azs", "ax", "axs")]).astype(rt).tofile(f)
        s.astype(rt).tofile(f)                                                       # T' x M x V in C order: pulse fastest, MATLAB's V x M x T'
        ext(np.zeros_like(cs["c"]) if ls is None else ls["kap"]).tofile(f)
        ext(F.nl_model(cs["rho"], cs["BoA"])["bq"]).tofile(f)
        if ls is None:
            np.array([float(_lib.FDTD_LOSS_STOKES)]).tofile(f)
        else:
            np.concatenate([[float(_lib.FDTD_LOSS_RELAX if L else _lib.FDTD_LOSS_STOKES)], ls["g"], ls["E"]]).astype(np.float64).tofile(f)
        np.stack([src_node.astype(np.float64), wz, wx], 1).tofile(f)
        sen_node.astype(np.float64).tofile(f)
    return len(sen_node), V


@pytest.mark.gpu
@pytest.mark.parametrize("double,L,convective", [(False, 3, True), (True, None, True), (True, 0, False), (False, None, False)],
                         ids=["single-L3", "double-lossless", "double-stokes-noconv", "single-lossless-noconv"])
def test_fdtdnl_command_matches_the_c_abi_and_the_python_layer(tmp_path, double, L, convective):
    from qups_amd import fdtd as F
    from tests import fdtd_loss_ref as LR
    from tests import fdtd_nl_ref as NR
    Z, X, P, R_ = 37, 29, 6, 4
    cs = NR.nl_case(Z, X, P, 3)
    ls = None if L is None else LR.loss_case(Z, X, L, cs["dt"])
    inp, dump = str(tmp_path / "case.bin"), str(tmp_path / "fdtdnl.bin")
    N, V = write_case(inp, cs, ls, R_, double, convective)
    r = subprocess.run([build_gateway(tmp_path), inp, dump], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fdtdnl gateway OK" in r.stdout, r.stdout + r.stderr
    assert "bit-identical to the C ABI" in r.stdout
    rt = np.float64 if double else np.float32
    mex = np.fromfile(dump, rt).reshape(V, N, cs["Nt"]).transpose(2, 1, 0)           # MATLAB's Nt x N x V, time fastest in the file
    pos = lambda w: np.stack([cs["z"][cs[w][0]], cs["x"][cs[w][1]]])
    loss = None if ls is None else dict(mode="relax" if L else "stokes", g=ls["g"], E=ls["E"], kap=ls["kap"])
    got = F.fdtd(cs["c"], cs["rho"], cs["z"], cs["x"], pos("src"), cs["nrm"], cs["s"], pos("sen"), cs["Nt"], cs["dt"], PML=P, order=2 * R_,
                 prec="double" if double else "single", loss=loss, BoA=cs["BoA"], convective=convective).cpu().numpy()
    assert got.shape == mex.shape and got.dtype == mex.dtype
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(mex).view(np.uint8))
