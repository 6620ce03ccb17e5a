"""qdas_fdtd_lossy without a GPU: the relaxation fit of qups_amd/fdtd.py (non-negative weights, ``fit_err`` reproduced from the discrete response, the
active-set solve against ``scipy.optimize.nnls`` where scipy imports), the restatement tests/fdtd_loss_ref.py against tests/fdtd_ref.py at zero loss, the
loss block against the header, the C entry's validation (``device = -1``: nothing reaches a HIP call), the wrapper's arithmetic and refusals, the kernels'
per-lane loops walked on the CPU by a stand-alone program under AddressSanitizer and UBSan (tests/fdtd_loss_core_host.cpp), and the physics of the
restatement: the absorption it measures between two sensors against ``a w^y``.

THE PHYSICS BOUND.  tests/fdtd_loss_ref.py ``physics_setup``: homogeneous 1540 m/s, h = lambda / 6 at 5 MHz, c dt / h = 0.2, order 8, a point source and two
sensors 10.01 mm apart in depth on a 225 x 21 grid with PML 20, 0.75 dB/(MHz^y cm).  The float64 restatement's largest deviation of
``-ln(|P2 / P1|_lossy / |P2 / P1|_lossless) / d`` from ``a w^y`` over 3 .. 7 MHz (41 frequencies) was measured once: 1.297 % (y = 1.1, L = 3), 1.399 %
(y = 1.5, L = 3), 1.376 % (Stokes) -- ``PHYS_DEV`` below; the fits' own errors are 0.04 % and 0.02 %, the rest is the grid's.  The tests assert TWICE those
values, here for the restatement and in tests/test_gpu_fdtd_loss.py for the device's record."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from qups_amd import DasError, Scan, Sequence, Transducer, UltrasoundSystem, _lib
from qups_amd import fdtd as F
from tests import fdtd_loss_ref as LR
from tests import fdtd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHYS_DEV = {(1.1, 3): 0.01297, (1.5, 3): 0.01399, (2.0, 0): 0.01376}       # measured on the float64 restatement (the module's docstring)
PHYS_FREQS = np.linspace(3e6, 7e6, 41)


# ---------------------------------------------------------------------------------------------------------------- the fit
FITS = [(1.01, 3), (1.1, 1), (1.1, 2), (1.1, 3), (1.5, 3), (1.5, 4), (1.8, 4), (1.0, 2)]
DTS = {"fine": 6.67e-9, "coarse": 1.6e-8}


@pytest.mark.parametrize("dt", list(DTS), ids=list(DTS))
@pytest.mark.parametrize("y,L", FITS)
def test_fit_weights_are_not_negative_and_fit_err_is_the_discrete_responses(y, L, dt):
    band, dt = (3e6, 7e6), DTS[dt]
    tau, E, g, fit_err = F.relaxation_fit(y, band, dt, L)
    assert tau.shape == E.shape == g.shape == (L,) and (g >= 0).all() and g.sum() > 0 and np.isfinite(g).all()
    assert np.allclose(E, 1.0 - np.exp(-dt / tau), rtol=1e-13) and ((E > 0) & (E <= 1)).all()
    fc = 1.0 / (2 * np.pi * tau)
    assert np.all(np.diff(fc) > 0) and fc[0] <= band[0] * (1 + 1e-12) or L == 1
    # fit_err again, from D_l = 1 - E_l / (1 - (1 - E_l) e^{i w dt}) written out here
    w = 2 * np.pi * np.geomspace(*band, 64)
    D = 1.0 - E[:, None] / (1.0 - (1.0 - E[:, None]) * np.exp(1j * w[None] * dt))
    dev = (g[:, None] * -D.imag).sum(0) / w ** (y - 1.0) - 1.0
    print(f"fdtd loss fit y = {y} L = {L} dt = {dt:g}: fit_err {fit_err:.3e}, centres {np.round(fc / 1e6, 2)} MHz")
    assert np.abs(dev).max() == pytest.approx(fit_err, rel=1e-9)
    if L >= 3:
        assert fit_err < 0.01, "three mechanisms follow the power law within 1 % inside the band"


def test_the_discrete_response_is_the_updates_own_and_tends_to_debye():
    """``e <- e + E (r - e)`` driven by ``r = e^{-i w n dt}``: the settled ``(r - e) / r`` is ``D``; for ``dt -> 0`` it is ``-i w tau / (1 - i w tau)``"""
    tau, dt, w = 4e-8, 1.6e-8, 2 * np.pi * 5e6
    E, D = F.relaxation_response([tau], dt, [w])
    e = 0j
    for n in range(400):
        r = np.exp(-1j * w * n * dt)
        e = e + E[0] * (r - e)
    assert (r - e) / r == pytest.approx(D[0, 0], rel=1e-10) and D[0, 0].imag < 0
    _, Df = F.relaxation_response([tau], 1e-13, [w])
    assert Df[0, 0] == pytest.approx(-1j * w * tau / (1 - 1j * w * tau), rel=1e-4)
    assert abs(D[0, 0].imag / Df[0, 0].imag - 1) > 0.02, "at this step the two differ by more than 2 %: the fit must use the discrete one"


def test_the_active_set_solve_agrees_with_scipys_nnls():
    nnls = pytest.importorskip("scipy.optimize").nnls
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 4):
        for _ in range(20):
            A, b = rng.standard_normal((64, n)), rng.standard_normal(64)
            want, rn = nnls(A, b)
            got = F._nnls_active_sets(A, b)
            assert (got >= 0).all() and np.linalg.norm(A @ got - b) == pytest.approx(rn, rel=1e-9, abs=1e-12)
            assert np.allclose(got, want, rtol=1e-7, atol=1e-10)
    # and on the fit's own matrix, where a column may be switched off
    w = 2 * np.pi * np.geomspace(3e6, 7e6, 64)
    _, D = F.relaxation_response(1.0 / (2 * np.pi * np.geomspace(0.5e6, 42e6, 4)), 6.67e-9, w)
    A = (-D.imag / (w / w.mean()) ** 0.8).T
    want, _ = nnls(A, np.ones(64))
    assert np.allclose(F._nnls_active_sets(A, np.ones(64)), want, rtol=1e-6, atol=1e-9)


def test_fit_refusals_and_the_unit_conversion():
    for bad in (dict(y=0.9), dict(y=2.0), dict(L=0), dict(L=5), dict(band=(0.0, 1e6)), dict(band=(2e6, 1e6)), dict(dt=0.0)):
        kw = dict(y=1.1, band=(3e6, 7e6), dt=1e-8, L=3)
        kw.update(bad)
        with pytest.raises(ValueError):
            F.relaxation_fit(kw["y"], kw["band"], kw["dt"], kw["L"])
    # 1 dB/(MHz cm) at y = 1: 100 / 8.685889638 Np/m at 1 MHz, i.e. per rad/s: / (2 pi 1e6)
    assert F.alpha_np(1.0, 1.0) == pytest.approx(100.0 / 8.685889638065035 / (2 * np.pi * 1e6), rel=1e-12)
    assert F.alpha_np(0.75, 2.0) * (2 * np.pi * 5e6) ** 2 == pytest.approx(0.75 * 25 * 100 / 8.685889638065035, rel=1e-12)


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("L", [0, 1, 3])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_zero_loss_is_the_lossless_restatement_bit_for_bit(L, dtype):
    cs = R.parity_case(37, 29, 6, 2)
    ls = LR.loss_case(37, 29, L, cs["dt"])
    args = (cs["c"], cs["rho"], cs["h"], cs["dt"], 6, 4, cs["src"], cs["nrm"], cs["s"], cs["sen"], cs["Nt"])
    want, ws = R.simulate(*args, dtype)
    got, gs = LR.simulate(*args, np.zeros((37, 29)), ls["g"], ls["E"], dtype)
    assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))
    for k in ws:
        assert np.array_equal(np.ascontiguousarray(gs[k]).view(np.uint8), np.ascontiguousarray(ws[k]).view(np.uint8)), k
    lossy, _ = LR.simulate(*args, ls["kap"], ls["g"], ls["E"], dtype)
    assert not np.array_equal(lossy, want) and np.isfinite(lossy).all()
    if L:
        assert np.abs(gs["e"]).max() > 0, "the memory variables follow rz + rx at every node, lossy or not"


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_loss_block_against_the_header():
    with open(os.path.join(ROOT, "include", "qdas.h")) as f:
        header = f.read()
    body = re.search(r"typedef struct qdas_fdtd_loss \{(.*?)\} qdas_fdtd_loss;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[\d+\]", "", n).strip(" *") for decl in body.split(";") if decl.strip()
             for n in re.sub(r"^(const\s+)?\w+\s", "", decl.strip()).split(",")]
    assert names == [n for n, _ in _lib.FdtdLoss._fields_] == ["mode", "L", "g", "E", "kap", "e"]
    assert C.sizeof(_lib.FdtdLoss) == 2 * 4 + 8 * 8 + 2 * 8 and _lib.FdtdLoss.g.offset == 8 and _lib.FdtdLoss.E.offset == 40 and _lib.FdtdLoss.kap.offset == 72
    for name, val in (("QDAS_FDTD_LOSS_STOKES", _lib.FDTD_LOSS_STOKES), ("QDAS_FDTD_LOSS_RELAX", _lib.FDTD_LOSS_RELAX), ("QDAS_FDTD_MAX_L", _lib.FDTD_MAX_L)):
        assert re.search(rf"#define {name} {val}\b", header)
    assert "qdas_fdtd_lossy" in _lib.SYMBOLS and hasattr(_lib.lib(), "qdas_fdtd_lossy")
    assert _lib.lib().qdas_fdtd_lossy.argtypes == [C.POINTER(_lib.FdtdDesc), C.POINTER(_lib.FdtdArgs), C.POINTER(_lib.FdtdLoss)]
    proto = re.search(r"\bint\s+qdas_fdtd_lossy\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1)
    assert "stream" not in proto and proto.count(",") == 2 and "qdas_fdtd_desc" in proto and "qdas_fdtd_loss" in proto


def _desc(**kw):
    d = _lib.FdtdDesc()
    base = dict(Nz=49, Nx=41, V=2, Nt=3, ld=49, vstride=49 * 41, M=1, Ts=2, N=1, rec_st=2, rec_sn=2, rec_sv=1, dt_h=0.3, inv_h=1e4, dtype=1, order=8, device=-1)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return d


def _args(**null):
    a = _lib.FdtdArgs()
    for n in _lib.FDTD_ARGS:
        setattr(a, n, None if null.get(n) else 0x1000)          # never dereferenced: every row below is refused on the host
    return a


def _loss(mode=_lib.FDTD_LOSS_RELAX, L=2, g=(0.5, 0.5), E=(0.1, 0.5), kap=0x1000, e=0x1000):
    q = _lib.FdtdLoss()
    q.mode, q.L, q.kap, q.e = mode, L, kap, e
    for k, v in enumerate(g):
        q.g[k] = v
    for k, v in enumerate(E):
        q.E[k] = v
    return q


def test_every_validation_row_of_the_lossy_entry():
    L = _lib.lib()
    last = lambda: L.qdas_last_error().decode()
    call = lambda d, a, q: L.qdas_fdtd_lossy(C.byref(d) if d is not None else None, C.byref(a) if a is not None else None, C.byref(q) if q is not None else None)
    assert call(None, None, None) == 1 and "null descriptor" in last()
    # the descriptor's rows are qdas_fdtd's
    for kw, code, msg in [(dict(dtype=2), 1, "dtype"), (dict(Nz=0), 1, "at least one node"), (dict(ld=48), 1, "ld = 48"), (dict(flags=2), 1, "unknown flags"),
                          (dict(order=6), 2, "order 6"), (dict(V=65536), 2, "65535"), (dict(dt_h=float("nan")), 1, "finite and positive")]:
        assert call(_desc(**kw), _args(), _loss()) == code and re.search(msg, last()), (kw, last())
    nan, inf = float("nan"), float("inf")
    rows = [(None, "null loss block"), (_loss(mode=0), "unknown loss mode 0"), (_loss(mode=3), "unknown loss mode 3"), (_loss(L=5, g=(0.2,) * 4, E=(0.2,) * 4), "L = 5"),
            (_loss(L=-1), "L = -1"), (_loss(L=0), "L = 0 with mode 2"), (_loss(mode=_lib.FDTD_LOSS_STOKES, L=1), "L = 1 with mode 1"),
            (_loss(g=(0.5, nan)), r"g\[1\]"), (_loss(g=(inf, 0.5)), r"g\[0\]"), (_loss(g=(0.5, -1e-9)), r"g\[1\]"),
            (_loss(E=(0.0, 0.5)), r"E\[0\]"), (_loss(E=(0.1, 1.0000001)), r"E\[1\]"), (_loss(E=(nan, 0.5)), r"E\[0\]"), (_loss(E=(-0.1, 0.5)), r"E\[0\]"),
            (_loss(kap=None), "null pointer \\(the loss"), (_loss(e=None), "null pointer \\(the loss"), (_loss(mode=_lib.FDTD_LOSS_STOKES, L=0, kap=None), "null pointer \\(the loss")]
    for q, msg in rows:
        assert call(_desc(), _args(), q) == 1 and re.search(msg, last()), (msg, last())
    assert call(_desc(), None, _loss()) == 1 and "null argument block" in last()
    for name in _lib.FDTD_ARGS:
        assert call(_desc(), _args(**{name: True}), _loss()) == 1 and "null pointer" in last(), (name, last())
    # nothing to do: QDAS_OK before any pointer is looked at, g = 0 and E = 1 are inside their ranges
    assert call(_desc(Nt=0), None, _loss(kap=None, e=None)) == 0 and call(_desc(V=0), None, _loss(g=(0.0, 0.0), E=(1.0, 1.0), kap=None, e=None)) == 0
    # but an empty call is still validated, the loss block included
    assert call(_desc(Nt=0, order=6), None, _loss()) == 2 and call(_desc(V=0), None, _loss(mode=7)) == 1 and call(_desc(Nt=0), None, None) == 1


def test_the_entry_keeps_the_rules_of_the_lossless_one():
    """the stream in the descriptor, no work space, no atomics, no graph, and still two launches per step: one host loop serves both entries"""
    from tests.test_scratch_host import scratch_users
    from tests.test_streams_host import stream_entries
    with open(os.path.join(ROOT, "include", "qdas.h")) as f:
        assert not [n for n in stream_entries(f.read()) if "fdtd" in n]
    with open(os.path.join(ROOT, "qups_amd", "csrc", "fdtd.hip")) as f:
        src = f.read()
    code = re.sub(r"//[^\n]*", "", src)
    assert not scratch_users(src) and "hipMalloc" not in src and "Synchronize" not in src and "atomic" not in code and "hipGraph" not in code
    assert len(re.findall(r"<<<", code)) == 2 and "density_lossy_kernel" in code and "density_cells_lossy" in code
    from tests import test_gpu_fdtd_loss as G
    assert callable(G.test_stream_delayed_producer_on_a_side_stream)


# ---------------------------------------------------------------------------------------------------------------- the wrapper
H, C0, FC = 1e-4, 1500.0, 2.5e6


def _system(Z=50, X=40, fs=10e6, y=None):
    z, x = np.arange(Z) * H, (np.arange(X) - (X - 1) / 2) * H
    if y is not None:
        return UltrasoundSystem(Transducer.matrix((2, 2), (0.3e-3, 0.3e-3), FC), Sequence("FSA", c0=C0), Scan.cartesian(x, z, y), fs=fs)
    return UltrasoundSystem(Transducer.linear(4, 0.3e-3, FC), Sequence("FSA", c0=C0), Scan.cartesian(x, z), fs=fs)


def test_the_time_step_respects_the_unrelaxed_speed_and_the_band_defaults_to_the_transducers():
    us = _system()
    c = np.full((50, 40), C0)
    kw = dict(waveform=np.ones(3), wv_t0=0.0, wv_fs=60e6, plan_only=True)
    plain = us.fdtdSim(c, **kw)
    assert "loss" not in plain and plain["ratio"] == 6
    # 5 dB/(MHz^1.1 cm) is strong: the fit gives kap sum g, and c sqrt(1 + kap sum g) must stay inside CFL_max
    plan = us.fdtdSim(c, alpha=5.0, alpha_power=1.1, **kw)
    ls = plan["loss"]
    assert ls["mode"] == "relax" and ls["L"] == 3 and ls["y"] == 1.1 and 0 < ls["fit_err"] < 0.01
    band = (0.5 * FC, 1.5 * FC)
    tau, E, g, err = F.relaxation_fit(1.1, band, plan["dt"], 3)
    assert np.array_equal(ls["g"], g) and np.array_equal(ls["E"], E) and ls["fit_err"] == err, "the fit in use is the one at the final dt"
    kap = 2 * C0 * F.alpha_np(5.0, 1.1)
    assert np.allclose(ls["kap"], kap, rtol=1e-14) and ls["speed"] == pytest.approx(C0 * np.sqrt(1 + kap * g.sum()), rel=1e-12)
    assert ls["speed"] > C0 and ls["speed"] * plan["dt"] / H <= 0.25 and plan["ratio"] >= plain["ratio"]
    assert plan["ratio"] == int(np.ceil(F.loss_model(c, 5.0, 1.1, band, plain["dt"], 3)["speed"] / (10e6 * 0.25 * H) - 1e-12))
    # a map, and the default power 1.01
    amap = np.zeros((50, 40))
    amap[20:] = 0.5
    plan = us.fdtdSim(c, alpha=amap, **kw)
    assert plan["loss"]["y"] == 1.01 and np.all(plan["loss"]["kap"][:20] == 0) and np.all(plan["loss"]["kap"][20:] > 0)
    # Stokes: no mechanisms, mud = 2 c a / dt
    plan = us.fdtdSim(c, alpha=0.5, alpha_power=2, **kw)
    assert plan["loss"]["mode"] == "stokes" and plan["loss"]["L"] == 0 and np.allclose(plan["loss"]["kap"], 2 * C0 * F.alpha_np(0.5, 2) / plan["dt"], rtol=1e-14)
    assert us.fdtdSim(c, alpha=0.5, alpha_power=1.5, alpha_band=(1e6, 3e6), mechanisms=2, **kw)["loss"]["L"] == 2


def test_refusals_of_the_wrapper():
    us = _system()
    c = np.full((50, 40), C0)
    kw = dict(waveform=np.ones(3), wv_t0=0.0, wv_fs=60e6, plan_only=True)
    for bad in (dict(alpha=0.5, alpha_power=0.9), dict(alpha=0.5, alpha_power=2.1), dict(alpha=-0.1), dict(alpha=np.full((50, 40), -1.0)), dict(alpha=float("nan")),
                dict(alpha=0.5, mechanisms=5), dict(alpha=0.5, mechanisms=0)):
        with pytest.raises(ValueError):
            us.fdtdSim(c, **bad, **kw)
    with pytest.raises(DasError, match="size"):
        us.fdtdSim(c, alpha=np.zeros((50, 41)), **kw)
    vol = _system(Z=12, X=10, y=np.arange(6) * H)
    with pytest.raises(NotImplementedError, match="2-D"):
        vol.fdtdSim(np.full((12, 10, 6), C0), alpha=0.5, **kw)
    z, x = np.arange(50) * H, (np.arange(40) - 19.5) * H
    none = np.zeros((2, 0))
    with pytest.raises(DasError, match="alpha_band"):
        F.fdtd(c, c, z, x, none, none, np.zeros((1, 0, 1)), none, 1, 1e-8, alpha=0.5, alpha_power=1.1)
    with pytest.raises(DasError, match="with absorption"):                             # c dt / h = 0.54 alone is inside the limit 0.5497
        F.fdtd(c, c, z, x, none, none, np.zeros((1, 0, 1)), none, 1, 0.54 * H / C0, alpha=20.0, alpha_power=1.1, alpha_band=(1e6, 4e6))


# ---------------------------------------------------------------------------------------------------------------- the device's core, on the host
@pytest.fixture(scope="module")
def core_exe(tmp_path_factory):
    """fdtd_core.h's lossy pass under AddressSanitizer and UBSan in a stand-alone program: LDS blocks, states, memory variables, tables and the record are heap
    blocks of exactly their size"""
    exe = str(tmp_path_factory.mktemp("fdl") / "fdtd_loss_core_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "qups_amd", "csrc"), os.path.join(ROOT, "tests", "fdtd_loss_core_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_core(exe, tmp_path, cs, ls, P, R_, double, ld_extra=0):
    tab = F.prepare(cs["c"], cs["rho"], cs["h"], cs["dt"], P)
    Nz, Nx = tab["Nz"], tab["Nx"]
    s = np.asarray(cs["s"], np.float64)
    Ts, M, V = s.shape
    h, dt, Nt = cs["h"], cs["dt"], cs["Nt"]
    src_node = ((np.asarray(cs["src"][1], np.int64) + P) * Nz + np.asarray(cs["src"][0], np.int64) + P).astype(np.int32)
    sen_node = ((np.asarray(cs["sen"][1], np.int64) + P) * Nz + np.asarray(cs["sen"][0], np.int64) + P).astype(np.int32)
    N, L = sen_node.size, len(ls["g"])
    nrm = np.asarray(cs["nrm"], np.float64).reshape(2, -1)
    csrc = tab["c"].reshape(-1)[src_node]
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        np.array([0 if double else 1, R_, Nz, Nx, V, Nt, Nz + ld_extra, M, Ts, N, L, 0], np.int64).tofile(f)
        np.array([dt / h, 1.0 / h]).tofile(f)
        for k in ("c2", "rho", "dtrz", "dtrx"):
            np.ascontiguousarray(tab[k], np.float64).tofile(f)
        np.ascontiguousarray(np.pad(ls["kap"], P, mode="edge").T, np.float64).tofile(f)
        for k in ("az", "azs", "ax", "axs"):
            np.ascontiguousarray(tab[k], np.float64).tofile(f)
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


def check(rec, st, r64, d32, double, what):
    worst = 0.0
    for name, g, want in [("rec", rec, r64[0])] + [(k, st[k], r64[1][k]) for k in (*F.STATES, "e")]:
        assert g.shape == want.shape, (name, g.shape, want.shape)
        if not want.size:
            continue
        err = np.abs(g - want).max() / np.abs(want).max()
        tol = R.tolerance(d32[name], double)
        worst = max(worst, err / tol)
        assert err <= tol, (what, name, err, tol)
    print(f"fdtd loss core {what}: largest err / tolerance {worst:.3f}")


@pytest.mark.parametrize("L", [0, 1, 4])
@pytest.mark.parametrize("R_", [1, 4])
@pytest.mark.parametrize("grid", [(37, 29, 6), (130, 3, 4)], ids=lambda g: "x".join(str(v) for v in g))
def test_the_lossy_core_on_the_host_matches_the_restatement(core_exe, tmp_path, grid, R_, L):
    """float32 for every case, float64 (with a padded row stride) for R = 4; V = 3"""
    cs, ls, r64, _, d32 = LR.parity_refs(*grid, R_, 3, L)
    for double in ((False, True) if R_ == 4 else (False,)):
        rec, st = run_core(core_exe, tmp_path, cs, ls, grid[2], R_, double, ld_extra=5 if double else 0)
        check(rec, st, r64, d32, double, f"{grid} R = {R_} L = {L} {'f64' if double else 'f32'}")


# ---------------------------------------------------------------------------------------------------------------- the physics of the restatement
_PHYS = {}


def physics_reference():
    """the lossless float64 record of the physics case, computed once"""
    if not _PHYS:
        ps = LR.physics_setup()
        c = np.full((ps["Z"], ps["X"]), LR.C0)
        rho = np.full_like(c, LR.RHO0)
        args = (c, rho, ps["h"], ps["dt"], ps["P"], ps["R"], ps["src"], ps["nrm"], ps["s"], ps["sen"], ps["Nt"])
        base, _ = R.simulate(*args)
        base.setflags(write=False)
        _PHYS.update(ps=ps, c=c, args=args, base=base)
    return _PHYS


@pytest.mark.parametrize("y,L", LR.YS)
def test_the_restatement_absorbs_by_the_power_law(y, L):
    ph = physics_reference()
    ps = ph["ps"]
    m = F.loss_model(ph["c"], LR.ALPHA_DB, y, LR.BAND, ps["dt"], max(L, 1))
    assert m["L"] == L and m["speed"] * ps["dt"] / ps["h"] < 0.25
    rec, _ = LR.simulate(*ph["args"], m["kap"], m["g"], m["E"])
    got = LR.measured_alpha(rec[:, :, 0], ph["base"][:, :, 0], ps["dt"], ps["d"], PHYS_FREQS)
    want = F.alpha_np(LR.ALPHA_DB, y) * (2 * np.pi * PHYS_FREQS) ** y
    dev = np.abs(got / want - 1).max()
    print(f"fdtd loss physics y = {y} L = {L}: fit_err {m['fit_err']:.3e}, alpha at 5 MHz {got[20]:.2f} Np/m (law {want[20]:.2f}), largest deviation {dev:.4%}, "
          f"bound {2 * PHYS_DEV[(y, L)]:.4%}")
    assert dev <= 2 * PHYS_DEV[(y, L)]
    assert got[20] > 0.9 * want[20] > 0
