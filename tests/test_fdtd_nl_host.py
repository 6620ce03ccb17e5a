"""qdas_fdtd_nonlinear without a GPU: the restatement tests/fdtd_nl_ref.py against tests/fdtd_ref.py and tests/fdtd_loss_ref.py at a zero block, how hard the
parity cases drive the medium, the nonlinear block against the header, the C entry's validation (``device = -1``: nothing reaches a HIP call), the rules the
entry keeps, the wrapper's arithmetic and refusals, the kernels' per-lane loops walked on the CPU by a stand-alone program under AddressSanitizer and UBSan
(tests/fdtd_nl_core_host.cpp), and the physics of the restatement: the second harmonic of a plane wave against Fubini's solution.

THE PARITY CASES (``fdtd_nl_ref.nl_case``) are tests/fdtd_ref.py's with the source tables scaled so that the largest ``|u| / c`` of the linear run is 4e-3 (the
tests hold 1e-3 .. 1e-2 for every nonlinear run) and a ``B/A`` map between 0 (over part of the grid) and 10.  Every case must differ from its linear run by
more than 100 x the parity tolerance of the float32 record: parity cannot pass with the terms missing.

THE HOST WALK compares BITS.  The device states the roundings of the nonlinear pass with fused operations; built with ``-DQDAS_FD_UNFUSED`` and without
contraction the same text rounds every product, which is the restatement's arithmetic operation for operation -- so the walk must give the restatement's
float64 (and float32) values exactly, not within a tolerance.

THE PHYSICS BOUND.  ``fdtd_nl_ref.physics_setup``: homogeneous 1500 m/s, 1000 kg/m^3, 16 points per wavelength at 2.5 MHz, c dt / h = 0.2, order 8; with
``dt / rho_sgx = 0`` every column is a 1-D line; a 16-cycle burst of 0.5 MPa (v0 = 0.333 m/s, 3-cycle ramps), sensors at 2, 10, 20 and 30 wavelengths,
``|P2| / |P1|`` from a DFT over the central 8 cycles against Fubini's ``B2 / B1``, ``Bn = 2 Jn(n sigma) / (n sigma)``, ``sigma = beta (v0 / c) k x`` (up to
0.167 at ``beta = 4``).  The float64 restatement's deviations were measured once -- ``PHYS_DEV`` below, in the order of the sensors:
    both terms,       B/A = 6, beta = 4:   -2.626 %  -0.641 %  -0.488 %  -0.566 %
    convective alone, B/A = 0, beta = 1:   -2.445 %  -0.549 %  -0.413 %  -0.516 %
    quadratic alone,  B/A = 6, beta = 3:   -2.666 %  -0.653 %  -0.499 %  -0.586 %
(2 wavelengths from the source the harmonic is 0.5 % of the fundamental and the burst's ramps still weigh on it).  The tests assert TWICE those values, sensor
by sensor, here for the restatement and in tests/test_gpu_fdtd_nl.py for the device's float32 record."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from qups_amd import DasError, _lib
from qups_amd import fdtd as F
from tests import fdtd_loss_ref as LR
from tests import fdtd_nl_ref as NR
from tests import fdtd_ref as R
from tests.test_fdtd_loss_host import _args, _desc, _loss, _system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# measured on the float64 restatement (the module's docstring): variant -> |deviation| per sensor of fdtd_nl_ref.SENSORS
PHYS_DEV = {"both": (0.02626, 0.00641, 0.00488, 0.00566), "convective": (0.02445, 0.00549, 0.00413, 0.00516), "quadratic": (0.02666, 0.00653, 0.00499, 0.00586)}
PARITY_GRIDS = [(37, 29, 6), (64, 64, 0), (3, 130, 4), (130, 3, 4)]
ORDERS = (1, 2, 4)
gid = lambda g: "x".join(str(v) for v in g)
same_bits = lambda a, b: a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("L", [None, 0, 3])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_zero_block_is_the_linear_restatement_bit_for_bit(L, dtype):
    """K = 0 and bq = 0: tests/fdtd_ref.py without absorption, tests/fdtd_loss_ref.py with it"""
    cs = R.parity_case(37, 29, 6, 2)
    args = (cs["c"], cs["rho"], cs["h"], cs["dt"], 6, 4, cs["src"], cs["nrm"], cs["s"], cs["sen"], cs["Nt"])
    if L is None:
        (want, ws), kw = R.simulate(*args, dtype), {}
    else:
        ls = LR.loss_case(37, 29, L, cs["dt"])
        kw = dict(kap=ls["kap"], g=ls["g"], E=ls["E"])
        want, ws = LR.simulate(*args, ls["kap"], ls["g"], ls["E"], dtype)
    got, gs = NR.simulate(*args, np.zeros((37, 29)), K=0.0, dtype=dtype, **kw)
    assert same_bits(got, want)
    for k in ws:
        assert same_bits(gs[k], ws[k]), k
    # each term on its own moves the result (at the amplitude of the linear cases: by little, but not by nothing)
    for K, bq in ((2.0, 0.0), (0.0, 5e-3)):
        other, _ = NR.simulate(*args, np.full((37, 29), bq), K=K, dtype=dtype, **kw)
        assert not np.array_equal(other, want) and np.isfinite(other).all()


@pytest.mark.parametrize("grid", PARITY_GRIDS, ids=gid)
def test_every_parity_case_is_driven_hard_enough_that_the_terms_matter(grid):
    """for every case of tests/test_gpu_fdtd_nl.py: 1e-3 <= max|u| / c <= 1e-2, and the record differs from the linear run of the same sources by more than
    100 x the parity tolerance"""
    for R_ in ORDERS:
        for V in (1, 3):
            for L in NR.LOSSES:
                cs, ls, r64, _, d32 = NR.parity_refs(*grid, R_, V, L)
                lin = NR.linear_record(*grid, R_, V, L)
                mach = r64[1]["mach"]
                diff = np.abs(r64[0] - lin).max() / np.abs(r64[0]).max()
                tol = R.tolerance(d32["rec"], False)
                print(f"fdtd nl drive {grid} R = {R_} V = {V} L = {L}: max|u| / c {mach:.3e}, |nonlinear - linear| / max {diff:.3e} = {diff / tol:.0f} x the tolerance {tol:.2e}")
                assert 1e-3 <= mach <= 1e-2
                assert diff > 100 * tol
                assert np.isfinite(r64[0]).all() and (cs["BoA"] == 0).any() and cs["BoA"].max() == pytest.approx(NR.BOA_MAX)


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_nonlinear_block_against_the_header():
    with open(os.path.join(ROOT, "include", "qdas.h")) as f:
        header = f.read()
    body = re.search(r"typedef struct qdas_fdtd_nl \{(.*?)\} qdas_fdtd_nl;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in re.sub(r"^(const\s+)?\w+\s", "", decl.strip()).split(",")]
    assert names == [n for n, _ in _lib.FdtdNl._fields_] == ["bq", "flags"]
    assert C.sizeof(_lib.FdtdNl) == 16 and _lib.FdtdNl.bq.offset == 0 and _lib.FdtdNl.flags.offset == 8 and _lib.FdtdNl.flags.size == 4
    assert re.search(rf"#define QDAS_FDTD_NL_NO_CONVECTIVE {_lib.FDTD_NL_NO_CONVECTIVE}\b", header) and _lib.FDTD_NL_NO_CONVECTIVE == 1
    assert "qdas_fdtd_nonlinear" in _lib.SYMBOLS and hasattr(_lib.lib(), "qdas_fdtd_nonlinear")
    assert _lib.lib().qdas_fdtd_nonlinear.argtypes == [C.POINTER(_lib.FdtdDesc), C.POINTER(_lib.FdtdArgs), C.POINTER(_lib.FdtdLoss), C.POINTER(_lib.FdtdNl)]
    proto = re.search(r"\bint\s+qdas_fdtd_nonlinear\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1)
    proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
    assert "stream" not in proto and proto.count(",") == 3 and all(t in proto for t in ("qdas_fdtd_desc", "qdas_fdtd_args", "qdas_fdtd_loss", "qdas_fdtd_nl"))
    # the shared blocks are used as they are
    assert C.sizeof(_lib.FdtdDesc) == 12 * 8 + 2 * 8 + 4 * 4 + 8 and C.sizeof(_lib.FdtdArgs) == 8 * len(_lib.FDTD_ARGS) and C.sizeof(_lib.FdtdLoss) == 88


def _nl(bq=0x1000, flags=0):
    q = _lib.FdtdNl()
    q.bq, q.flags = bq, flags
    return q


def test_every_validation_row_of_the_nonlinear_entry():
    L = _lib.lib()
    last = lambda: L.qdas_last_error().decode()
    ref = lambda x: C.byref(x) if x is not None else None
    call = lambda d, a, l, q: L.qdas_fdtd_nonlinear(ref(d), ref(a), ref(l), ref(q))
    assert call(None, None, None, None) == 1 and "null descriptor" in last()
    # the descriptor's rows are qdas_fdtd's, with and without a loss block
    for l in (None, _loss()):
        for kw, code, msg in [(dict(dtype=2), 1, "dtype"), (dict(Nz=0), 1, "at least one node"), (dict(Nx=0), 1, "at least one node"), (dict(ld=48), 1, "ld = 48"),
                              (dict(vstride=49 * 41 - 1), 1, "vstride"), (dict(flags=2), 1, "unknown flags"), (dict(order=6), 2, "order 6"), (dict(V=65536), 2, "65535"),
                              (dict(dt_h=float("nan")), 1, "finite and positive"), (dict(inv_h=0.0), 1, "finite and positive"), (dict(Nz=2 ** 31), 1, "ld = "),
                              (dict(Nz=2 ** 31, ld=2 ** 31, vstride=2 ** 38), 2, "2\\^31"), (dict(M=2 ** 31), 2, "2\\^31"), (dict(Nt=2 ** 40), 2, "2\\^40")]:
            assert call(_desc(**kw), _args(), l, _nl()) == code and re.search(msg, last()), (kw, last())
    # the loss block's rows are qdas_fdtd_lossy's
    nan, inf = float("nan"), float("inf")
    rows = [(_loss(mode=0), "unknown loss mode 0"), (_loss(mode=3), "unknown loss mode 3"), (_loss(L=5, g=(0.2,) * 4, E=(0.2,) * 4), "L = 5"), (_loss(L=-1), "L = -1"),
            (_loss(L=0), "L = 0 with mode 2"), (_loss(mode=_lib.FDTD_LOSS_STOKES, L=1), "L = 1 with mode 1"), (_loss(g=(0.5, nan)), r"g\[1\]"),
            (_loss(g=(inf, 0.5)), r"g\[0\]"), (_loss(g=(0.5, -1e-9)), r"g\[1\]"), (_loss(E=(0.0, 0.5)), r"E\[0\]"), (_loss(E=(0.1, 1.0000001)), r"E\[1\]"),
            (_loss(E=(nan, 0.5)), r"E\[0\]"), (_loss(E=(-0.1, 0.5)), r"E\[0\]"), (_loss(kap=None), "null pointer \\(the loss"), (_loss(e=None), "null pointer \\(the loss"),
            (_loss(mode=_lib.FDTD_LOSS_STOKES, L=0, kap=None), "null pointer \\(the loss")]
    for l, msg in rows:
        assert call(_desc(), _args(), l, _nl()) == 1 and re.search(msg, last()), (msg, last())
    # the nonlinear block's own rows
    for l in (None, _loss()):
        assert call(_desc(), _args(), l, None) == 1 and "null nonlinear block" in last()
        assert call(_desc(), _args(), l, _nl(flags=2)) == 1 and "unknown flags 0x2" in last()
        assert call(_desc(), _args(), l, _nl(flags=-1)) == 1 and "unknown flags" in last()
        assert call(_desc(), _args(), l, _nl(bq=None)) == 1 and "null pointer (the nonlinearity map)" in last()
        assert call(_desc(), _args(), l, _nl(bq=None, flags=_lib.FDTD_NL_NO_CONVECTIVE)) == 1 and "nonlinearity map" in last()
        assert call(_desc(), None, l, _nl()) == 1 and "null argument block" in last()
        for name in _lib.FDTD_ARGS:
            assert call(_desc(), _args(**{name: True}), l, _nl()) == 1 and "null pointer" in last(), (name, last())
    # nothing to do: QDAS_OK after validation, before any pointer is looked at
    assert call(_desc(Nt=0), None, None, _nl(bq=None)) == 0 and call(_desc(V=0), None, _loss(kap=None, e=None), _nl(bq=None, flags=1)) == 0
    assert call(_desc(Nt=0, order=6), None, None, _nl()) == 2 and call(_desc(V=0), None, _loss(mode=7), _nl()) == 1
    assert call(_desc(Nt=0), None, None, None) == 1 and call(_desc(V=0), None, None, _nl(flags=4)) == 1


def test_the_entry_keeps_the_rules_of_the_lossless_one():
    """the stream in the descriptor, no work space, no atomics, no graph, no allocation, no synchronisation, and still two launches per step: one host loop
    serves the three entries, and the nonlinear density kernel goes through it as its density-kernel argument"""
    from tests.test_scratch_host import scratch_users
    from tests.test_streams_host import stream_entries
    with open(os.path.join(ROOT, "include", "qdas.h")) as f:
        assert not [n for n in stream_entries(f.read()) if "fdtd" in n]
    with open(os.path.join(ROOT, "qups_amd", "csrc", "fdtd.hip")) as f:
        src = f.read()
    code = re.sub(r"//[^\n]*", "", src)
    assert not scratch_users(src) and "hipMalloc" not in src and "Synchronize" not in src and "atomic" not in code and "hipGraph" not in code
    assert len(re.findall(r"<<<", code)) == 2 and "density_nl_kernel" in code and "density_cells_nl" in code
    assert re.search(r"run<R, T>\(P, s, Nt, Ts, density_nl_kernel<R, T, 0>, Q, N\)", code)
    assert "(hipStream_t)d->queue" in code.split('extern "C" int qdas_fdtd_nonlinear')[1]
    # the existing kernels' text is still there
    assert "density_lossy_kernel" in code and "density_cells_lossy" in code and "density_cells<R, T>" in code
    from tests import test_gpu_fdtd_nl as G
    assert callable(G.test_stream_delayed_producer_on_a_side_stream)


# ---------------------------------------------------------------------------------------------------------------- the wrapper
def test_the_nonlinear_block_of_the_wrapper():
    rho = np.array([[1000.0, 900.0], [1100.0, 1000.0]])
    m = F.nl_model(rho, 6.0)
    assert np.array_equal(m["bq"], 6.0 / (2.0 * rho)) and m["convective"] is True and m["beta_max"] == 4.0
    boa = np.array([[0.0, 5.0], [10.0, 7.0]])
    m = F.nl_model(rho, boa, convective=False)
    assert np.array_equal(m["bq"], boa / (2.0 * rho)) and m["convective"] is False and m["beta_max"] == 5.0
    # B/A = 0 is still nonlinear: beta = 1 from the convective term
    m = F.nl_model(rho, 0.0)
    assert m is not None and not m["bq"].any() and m["beta_max"] == 1.0
    assert F.nl_model(rho, None) is None and F.nl_model(rho, float("nan")) is None and F.nl_model(rho, np.full((2, 2), np.nan)) is None
    for bad in (np.array([[np.nan, 5.0], [1.0, 1.0]]), -1.0, np.array([[1.0, -1e-9], [1.0, 1.0]]), float("inf"), np.array([[1.0, np.inf], [1.0, 1.0]])):
        with pytest.raises(ValueError, match="BoA"):
            F.nl_model(rho, bad)
    with pytest.raises(DasError, match="size"):
        F.nl_model(rho, np.zeros((2, 3)))
    assert F.source_mach(np.array([[[0.2, -0.5]]]), np.array([1400.0, 1600.0]), 1e-8, 1e-4) == pytest.approx(0.5 * 2 * 1600.0 * 1e-8 / 1e-4 / 1400.0, rel=1e-14)
    assert F.source_mach(np.zeros((0, 2, 1)), np.array([1500.0]), 1e-8, 1e-4) == 0.0


def test_the_plan_of_fdtdsim_with_and_without_BoA():
    us = _system()
    c = np.full((50, 40), 1500.0)
    c[30:] = 1600.0
    wave = 0.3 * np.array([0.0, 1.0, -1.0, 0.5])
    kw = dict(waveform=wave, wv_t0=0.0, wv_fs=60e6, plan_only=True)
    plain = us.fdtdSim(c, **kw)
    assert "nl" not in plain
    for none in (None, float("nan"), np.full((50, 40), np.nan)):
        assert "nl" not in us.fdtdSim(c, BoA=none, **kw)
    plan = us.fdtdSim(c, BoA=6.0, **kw)
    # the time step is the linear one, and so is everything else of the plan
    assert all(plan[k] == plain[k] for k in ("h", "ratio", "fs_", "dt", "txn0", "txne", "Nt", "t0", "P", "Nz", "Nx", "T")) and "loss" not in plan
    s, _, _ = F.tx_table(wave, 0.0, 60e6, us.seq.delays(us.tx), us.seq.apodization(us.tx), plan["fs_"])
    assert plan["nl"]["beta_max"] == 4.0
    assert plan["nl"]["mach"] == pytest.approx(np.abs(s).max() * 2 * 1600.0 * plan["dt"] / plan["h"] / 1500.0, rel=1e-13) and plan["nl"]["mach"] > 0
    assert np.array_equal(plan["nl"]["bq"], 6.0 / (2.0 * plan["rho"]))
    boa = np.zeros((50, 40))
    boa[25:] = 9.0
    rho = np.full((50, 40), 1000.0)
    rho[:, 20:] = 1100.0
    plan = us.fdtdSim(c, rho, BoA=boa, **kw)
    assert plan["nl"]["beta_max"] == 5.5 and np.array_equal(plan["nl"]["bq"], boa / (2.0 * rho))
    assert us.fdtdSim(c, BoA=0.0, **kw)["nl"]["beta_max"] == 1.0
    # with absorption: both blocks, the time step of the lossy plan
    lossy = us.fdtdSim(c, alpha=0.5, alpha_power=1.1, **kw)
    both = us.fdtdSim(c, alpha=0.5, alpha_power=1.1, BoA=6.0, **kw)
    assert both["dt"] == lossy["dt"] and both["loss"]["L"] == 3 and both["nl"]["beta_max"] == 4.0 and np.array_equal(both["loss"]["g"], lossy["loss"]["g"])


def test_refusals_of_the_wrapper():
    us = _system()
    c = np.full((50, 40), 1500.0)
    kw = dict(waveform=np.ones(3), wv_t0=0.0, wv_fs=60e6, plan_only=True)
    part = np.full((50, 40), 6.0)
    part[3, 4] = np.nan
    for bad in (part, -0.5, np.full((50, 40), -1.0), float("inf"), np.where(np.arange(40) == 7, np.inf, 1.0) * np.ones((50, 1))):
        with pytest.raises(ValueError, match="BoA"):
            us.fdtdSim(c, BoA=bad, **kw)
    with pytest.raises(DasError, match="size"):
        us.fdtdSim(c, BoA=np.zeros((50, 41)), **kw)
    vol = _system(Z=12, X=10, y=np.arange(6) * 1e-4)
    with pytest.raises(NotImplementedError, match="2-D"):
        vol.fdtdSim(np.full((12, 10, 6), 1500.0), BoA=6.0, **kw)
    assert "nl" not in vol.fdtdSim(np.full((12, 10, 6), 1500.0), **kw)
    z, x = np.arange(50) * 1e-4, (np.arange(40) - 19.5) * 1e-4
    none = np.zeros((2, 0))
    with pytest.raises(ValueError, match="BoA"):                 # (before any device work)
        F.fdtd(c, c, z, x, none, none, np.zeros((1, 0, 1)), none, 1, 1e-8, BoA=part)


# ---------------------------------------------------------------------------------------------------------------- the device's core, on the host
@pytest.fixture(scope="module")
def core_exe(tmp_path_factory):
    """fdtd_core.h's nonlinear pass under AddressSanitizer and UBSan in a stand-alone program: LDS blocks, states, memory variables, tables and the record are
    heap blocks of exactly their size"""
    exe = str(tmp_path_factory.mktemp("fdn") / "fdtd_nl_core_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-DQDAS_FD_UNFUSED", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "qups_amd", "csrc"), os.path.join(ROOT, "tests", "fdtd_nl_core_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_core(exe, tmp_path, cs, ls, P, R_, double, K=2.0, ld_extra=0):
    tab = F.prepare(cs["c"], cs["rho"], cs["h"], cs["dt"], P)
    Nz, Nx = tab["Nz"], tab["Nx"]
    s = np.asarray(cs["s"], np.float64)
    Ts, M, V = s.shape
    h, dt, Nt = cs["h"], cs["dt"], cs["Nt"]
    src_node = ((np.asarray(cs["src"][1], np.int64) + P) * Nz + np.asarray(cs["src"][0], np.int64) + P).astype(np.int32)
    sen_node = ((np.asarray(cs["sen"][1], np.int64) + P) * Nz + np.asarray(cs["sen"][0], np.int64) + P).astype(np.int32)
    N, L = sen_node.size, (0 if ls is None else len(ls["g"]))
    nrm = np.asarray(cs["nrm"], np.float64).reshape(2, -1)
    csrc = tab["c"].reshape(-1)[src_node]
    ext = lambda m: np.ascontiguousarray(np.pad(m, P, mode="edge").T, np.float64)
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        np.array([0 if double else 1, R_, Nz, Nx, V, Nt, Nz + ld_extra, M, Ts, N, L, 0 if ls is None else 1], np.int64).tofile(f)
        np.array([dt / h, 1.0 / h, K]).tofile(f)
        for k in ("c2", "rho", "dtrz", "dtrx"):
            np.ascontiguousarray(tab[k], np.float64).tofile(f)
        ext(np.zeros_like(cs["c"]) if ls is None else ls["kap"]).tofile(f)
        ext(cs["bq"]).tofile(f)
        for k in ("az", "azs", "ax", "axs"):
            np.ascontiguousarray(tab[k], np.float64).tofile(f)
        if ls is not None:
            np.asarray(ls["g"], np.float64).tofile(f)
            np.asarray(ls["E"], np.float64).tofile(f)
        np.ascontiguousarray(s).tofile(f)
        (nrm[0] * 2.0 * csrc * dt / h).tofile(f)
        (nrm[1] * 2.0 * csrc * dt / h).tofile(f)
        src_node.tofile(f)
        sen_node.tofile(f)
    r = subprocess.run([exe, inp, out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    raw = np.fromfile(out)
    nr, ns = Nt * N * V, 5 * V * Nx * Nz
    assert raw.size == nr + ns + V * L * Nx * Nz
    st = dict(zip(F.STATES, raw[nr:nr + ns].reshape(5, V, Nx, Nz).transpose(0, 1, 3, 2)))
    st["e"] = raw[nr + ns:].reshape(V, L, Nx, Nz).transpose(0, 1, 3, 2)
    return raw[:nr].reshape(Nt, N, V), st


@pytest.mark.parametrize("L", NR.LOSSES, ids=lambda L: f"L{L}")
@pytest.mark.parametrize("R_", ORDERS)
@pytest.mark.parametrize("grid", PARITY_GRIDS, ids=gid)
def test_the_nonlinear_core_on_the_host_gives_the_bits_of_the_restatement(core_exe, tmp_path, grid, R_, L):
    """float64 for every case (with a padded row stride at R = 4), float32 too at R = 4; V = 3.  ``L``: None without a loss block, 0 Stokes, 3 relaxation."""
    cs, ls, r64, r32, _ = NR.parity_refs(*grid, R_, 3, L)
    for double in ((True, False) if R_ == 4 else (True,)):
        rec, st = run_core(core_exe, tmp_path, cs, ls, grid[2], R_, double, ld_extra=5 if R_ == 4 and double else 0)
        want = r64 if double else r32
        assert np.array_equal(rec, want[0].astype(np.float64)), (grid, R_, L, double, "rec", np.abs(rec - want[0]).max())
        for k in (*F.STATES, "e"):
            assert np.array_equal(st[k], want[1][k].astype(np.float64)), (grid, R_, L, double, k)


def test_the_core_without_the_convective_term_and_with_a_zero_map(core_exe, tmp_path):
    """K = 0 (rho + 0 ro), and then a zero bq as well: the bits of the restatement, which at the zero block are the linear restatement's"""
    grid, R_ = (37, 29, 6), 4
    for L in (None, 3):
        cs, ls, r64, _, _ = NR.parity_refs(*grid, R_, 3, L, K=0.0)
        rec, st = run_core(core_exe, tmp_path, cs, ls, grid[2], R_, True, K=0.0)
        assert np.array_equal(rec, r64[0]) and all(np.array_equal(st[k], r64[1][k]) for k in (*F.STATES, "e"))
        args = (cs["c"], cs["rho"], cs["h"], cs["dt"], grid[2], R_, cs["src"], cs["nrm"], cs["s"], cs["sen"], cs["Nt"])
        want, ws = R.simulate(*args) if ls is None else LR.simulate(*args, ls["kap"], ls["g"], ls["E"])
        rec, st = run_core(core_exe, tmp_path, dict(cs, bq=np.zeros_like(cs["c"])), ls, grid[2], R_, True, K=0.0)
        assert np.array_equal(rec, want) and all(np.array_equal(st[k], ws[k]) for k in ws)


# ---------------------------------------------------------------------------------------------------------------- the physics of the restatement
# variant -> (K, the column of fdtd_nl_ref.COLUMNS it is read from, beta)
VARIANTS = {"both": (2.0, 0, 1.0 + NR.BOA / 2.0), "convective": (2.0, 1, 1.0), "quadratic": (0.0, 0, NR.BOA / 2.0)}
_PHYS = {}


def physics_records(K):
    """the float64 record of the physics case with the convective term (``K = 2``: columns B/A = 6 and B/A = 0) or without it, computed once"""
    if K not in _PHYS:
        ps = NR.physics_setup()
        rec, st = NR.simulate(ps["c"], ps["rho"], ps["h"], ps["dt"], ps["P"], ps["R"], ps["src"], ps["nrm"], ps["s"], ps["sen"], ps["Nt"], ps["BoA"] / (2.0 * ps["rho"]),
                              K=K, lines=True)
        rec.setflags(write=False)
        _PHYS[K] = (ps, rec[:, :, 0], st["mach"])
    return _PHYS[K]


def check_fubini(name, rec, ps, what):
    K, col, beta = VARIANTS[name]
    n = len(NR.SENSORS)
    for b, wl in enumerate(NR.SENSORS):
        got = NR.harmonic_ratio(rec[:, col * n + b], ps["spp"], wl)
        want = NR.fubini_ratio(beta, ps["v0"], wl)
        dev = got / want - 1.0
        print(f"fdtd nl physics ({what}) {name} beta = {beta:g} at {wl} wavelengths: |P2 / P1| {got:.6f}, Fubini {want:.6f}, deviation {dev:+.4%}, "
              f"bound {2 * PHYS_DEV[name][b]:.4%}")
        assert abs(dev) <= 2 * PHYS_DEV[name][b], (name, wl, dev)


@pytest.mark.parametrize("name", list(VARIANTS))
def test_the_restatement_follows_fubini(name):
    ps, rec, mach = physics_records(VARIANTS[name][0])
    assert mach == pytest.approx(ps["v0"] / NR.C0, rel=0.05), "a line of sources s = v0 radiates v0 each way"
    assert np.abs(rec[:, 0]).max() == pytest.approx(NR.P0, rel=0.03), "and rho c v0 of pressure"
    check_fubini(name, rec, ps, "restatement, float64")


def test_without_either_term_there_is_no_second_harmonic():
    """the control of the physics tests: the quadratic-alone run's B/A = 0 column is linear, and its second harmonic is that of the burst's ramps alone"""
    ps, rec, _ = physics_records(0.0)
    n = len(NR.SENSORS)
    for b, wl in enumerate(NR.SENSORS):
        assert NR.harmonic_ratio(rec[:, n + b], ps["spp"], wl) < 1e-5
