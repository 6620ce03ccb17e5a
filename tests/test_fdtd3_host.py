"""qdas_fdtd3 without a GPU: the physics of the restatement tests/fdtd3_ref.py (arrival lag and amplitude along the three axes, the order of the scheme, the
PML, the x <-> y swap), the wrapper arithmetic of qups_amd/fdtd3.py and of ``UltrasoundSystem.fdtdSim`` on a volume, the descriptor against the header, the
C entry's validation (``device = -1``: nothing reaches a HIP call), and the kernels' per-lane loops (``csrc/fdtd3_core.h``) walked on the CPU by a
stand-alone program under AddressSanitizer and UBSan (tests/fdtd3_core_host.cpp) against the restatement, within the GPU test's tolerance."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from qups_amd import DasError, Scan, Sequence, Transducer, UltrasoundSystem, _lib
from qups_amd import fdtd as F
from qups_amd import fdtd3 as F3
from tests import fdtd3_ref as R3
from tests.test_streams_host import stream_entries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---------------------------------------------------------------------------------------------------------------- the physics of the restatement
H, C0, RHO0, FC = 1e-4, 1500.0, 1000.0, 2.5e6
DT = 0.25 * H / C0


def _burst(dt):
    t = np.arange(0, 4.0 / FC, dt)
    tc = t.mean()
    return np.sin(2 * np.pi * FC * (t - tc)) * np.exp(-((t - tc) / (0.6 / FC)) ** 2)


def _along(axis, shape3, idx):
    """``idx`` along ``axis`` and the middle of the two other axes: an (iz, ix, iy) triple of arrays"""
    return tuple(np.asarray(idx) if a == axis else np.full(len(idx), shape3[a] // 2) for a in range(3))


@functools.lru_cache(maxsize=None)
def _axis_run(R_, axis):
    """a point source (its normal along ``axis``) 4 nodes into a 96 x 13 x 13 bar along ``axis``, PML 8; sensors 10 and 80 nodes on: (lag, far / near peak)"""
    shape3 = tuple(96 if a == axis else 13 for a in range(3))
    c = np.full(shape3, C0)
    nrm = np.zeros((3, 1))
    nrm[axis] = 1.0
    rec, _ = R3.simulate(c, np.full(shape3, RHO0), H, DT, 8, R_, _along(axis, shape3, [4]), nrm, _burst(DT)[:, None, None], _along(axis, shape3, [14, 84]), 520)
    return R3.xcorr_lag(rec[:, 0, 0], rec[:, 1, 0]), float(np.abs(rec[:, 1, 0]).max() / np.abs(rec[:, 0, 0]).max())


def test_arrival_lag_amplitude_and_the_order_of_the_scheme():
    """70 h / (c0 dt) = 280 samples between the sensors 10 and 80 nodes from the source.  This restatement gives 278.81 (-0.43 %) at R = 4 and 281.89 (+0.68 %)
    at R = 2 (6 points per wavelength at c dt / h = 0.25: the leapfrog step makes the eighth-order scheme early, space dispersion makes the fourth-order one
    late), and a far / near peak ratio of 0.1175 at R = 4 against 10 / 80 = 0.125 of 1 / r (the source is a dipole along the axis: on the axis its far field
    falls as 1 / r).  Bounds: within 1 % of the geometric lag, R = 4 early and R = 2 late; the amplitude ratio within 15 % of 1 / r."""
    l4, a4 = _axis_run(4, 0)
    l2, _ = _axis_run(2, 0)
    print(f"fdtd3 lag along z: R = 4 {l4:.2f} ({100 * (l4 / 280 - 1):+.2f} %), R = 2 {l2:.2f} ({100 * (l2 / 280 - 1):+.2f} %); far / near {a4:.4f}")
    assert abs(l4 - 280.0) <= 2.8 and abs(l2 - 280.0) <= 2.8
    assert l4 < 280.0 < l2
    assert abs(a4 / 0.125 - 1) <= 0.15


@pytest.mark.parametrize("axis", [1, 2])
def test_the_three_axes_agree(axis):
    (lz, az), (la, aa) = _axis_run(4, 0), _axis_run(4, axis)
    print(f"fdtd3 lag along {R3.AXES[axis]}: {la:.6f} against z {lz:.6f}; far / near {aa:.6f} against {az:.6f}")
    assert abs(la - lz) <= 1e-9 * lz and abs(aa - az) <= 1e-9 * az


@functools.lru_cache(maxsize=None)
def _late(P):
    shape3 = (41, 31, 31)
    c = np.full(shape3, C0)
    rec, _ = R3.simulate(c, np.full(shape3, RHO0), H, DT, P, 4, _along(0, shape3, [4]), [[1.0], [0.0], [0.0]], _burst(DT)[:, None, None], _along(0, shape3, [30]), 900)
    return float(np.abs(rec[500:]).max()), float(np.abs(rec[:500]).max())


def test_the_pml_absorbs():
    """a box of 41 x 31 x 31 nodes, the source 4 and the sensor 30 nodes deep on the axis, 900 steps: the late window (step >= 500) over the direct pulse is
    +2.9 dB in the rigid box (P = 0) and -83.7 dB with P = 10.  Bounds: at least 0 dB without a layer (nothing leaves a rigid box), at most -60 dB with it."""
    db = {P: 20 * np.log10(_late(P)[0] / _late(P)[1]) for P in (0, 10)}
    print(f"fdtd3 pml: late / direct {db[0]:+.1f} dB at P = 0, {db[10]:+.1f} dB at P = 10")
    assert db[0] >= 0.0
    assert db[10] <= -60.0


def test_the_axis_swap_reproduces_the_record():
    cs = R3.parity_case(*R3.GRIDS[0], 2)
    a, sa = R3.run_case(cs, 4)
    b, sb = R3.run_case(R3.swap_xy(cs), 4)
    err = np.abs(a - b).max() / np.abs(a).max()
    print(f"fdtd3 swap x <-> y: {err:.2e}")
    assert err <= 1e-12
    assert np.abs(sa["ux"] - sb["uy"].transpose(0, 1, 3, 2)).max() <= 1e-12 * np.abs(sa["ux"]).max()


# ---------------------------------------------------------------------------------------------------------------- wrapper arithmetic
def test_stability_limits_and_spacing():
    assert [round(F3.stability_limit(r), 4) for r in (1, 2, 4)] == [0.5774, 0.4949, 0.4488]
    assert all(F3.stability_limit(r) == pytest.approx(R3.limit(r), rel=1e-15) for r in (1, 2, 4))
    ax = np.arange(4) * H
    assert F3.grid_spacing3(ax, ax, ax + 3e-3) == pytest.approx(H, rel=1e-12)
    for bad in ((ax, ax, 2 * ax), (ax, 2 * ax, ax), (2 * ax, ax, ax), (np.array([0, 1, 2, 3.001]) * H, ax, ax)):
        with pytest.raises(DasError, match="uniform"):
            F3.grid_spacing3(*bad)
    with pytest.raises(DasError, match="two nodes"):
        F3.grid_spacing3(ax, ax, ax[:1])
    c = np.full((6, 5, 4), C0)
    none3 = np.zeros((3, 0))
    with pytest.raises(DasError, match="stability limit"):            # 0.46 > 0.4488, inside the 2-D limit 0.5497: refused before any device work
        F3.fdtd3(c, c, np.arange(6) * H, np.arange(5) * H, np.arange(4) * H, none3, none3, np.zeros((1, 0, 1)), none3, 1, 0.46 * H / C0, PML=0)
    assert F.pml_size([10, 14], 101, 101, 101) == 12 and F.pml_size([10, 14], 100, 108, 100) == 10 and F.pml_size(7, 5, 6, 7) == 7
    # Y + 2P decides: Z = X = 100 (120 .. 128 -> 5, 61, 31, 7, 2: P = 14), Y = 99: 119 -> 17, 121 -> 11, 123 -> 41, 125 -> 5, 127 -> 127: max 17, 61, 41, 7, 127
    assert F.pml_size([10, 14], 100, 100) == 14 and F.pml_size([10, 14], 100, 100, 99) == 13


def test_nearest_nodes3_and_prepare():
    z, x, y = np.arange(5) * 1e-3, np.arange(-3, 4) * 1e-3, np.arange(-1, 2) * 1e-3
    iz, ix, iy = F3.nearest_nodes3(z, x, y, np.array([[-2.9e-3, 0.4e-3, 3e-3], [0.9e-3, -0.2e-3, -5e-3], [0.0, 1.6e-3, 9e-3]]))
    assert iz.tolist() == [0, 2, 4] and ix.tolist() == [0, 3, 6] and iy.tolist() == [2, 1, 0]
    F3.nearest_nodes3(z, x, y, np.array([[0.0, 0.0], [-1e-3, 1e-3], [0.0, 0.0]]))                # the same (z, x), another y: distinct nodes
    with pytest.raises(DasError, match="Elements are not unique; the Scan spacing or sizing may be too small."):
        F3.nearest_nodes3(z, x, y, np.array([[0.1e-3, 0.3e-3], [0.1e-3, -0.1e-3], [0.0, 0.0]]))
    rng = np.random.default_rng(0)
    c, rho = rng.uniform(1400, 1600, (4, 3, 2)), rng.uniform(900, 1100, (4, 3, 2))
    tab = F3.prepare(c, rho, H, 1e-8, 2)
    ce, re_, sg, A = R3.tables(c, rho, H, 1e-8, 2)
    assert (tab["Nz"], tab["Nx"], tab["Ny"]) == (8, 7, 6) and tab["c2"].shape == (6, 7, 8)
    assert np.array_equal(tab["c2"], (ce * ce).transpose(2, 1, 0)) and np.array_equal(tab["rho"], re_.transpose(2, 1, 0))
    for k, g in zip(("dtrz", "dtrx", "dtry"), sg):
        assert np.array_equal(tab[k], (1e-8 / g).transpose(2, 1, 0))
    assert tab["dtry"][-1, 3, 3] == 1e-8 / re_[3, 3, -1] and tab["dtry"][0, 3, 3] == 1e-8 / (0.5 * (re_[3, 3, 0] + re_[3, 3, 1]))
    for k, (a, a_s) in zip(("z", "x", "y"), A):
        assert np.allclose(tab["a" + k], a, rtol=1e-15) and np.allclose(tab["a" + k + "s"], a_s, rtol=1e-15)
    with pytest.raises(DasError, match="one shape"):
        F3.prepare(c[:, :, 0], rho[:, :, 0], H, 1e-8, 2)


def test_brick_lists_hold_every_point_exactly_once():
    TZ, TX, TY = F3.BRICK
    assert (_lib.FDTD3_TZ, _lib.FDTD3_TX, _lib.FDTD3_TY) == (R3.TZ, R3.TX, R3.TY) == F3.BRICK and TZ == 64 and TX in (8, 16) and TY in (8, 16, 32)
    Nz, Nx, Ny = 2 * TZ + 10, 3 * TX + 1, 2 * TY + 1
    rng = np.random.default_rng(1)
    nodes = rng.choice(Nz * Nx * Ny, 400, replace=False).astype(np.int32)
    nodes[:4] = [0, Nz * Nx * Ny - 1, (TY * Nx + TX) * Nz + TZ, ((TY - 1) * Nx + TX - 1) * Nz + TZ - 1]
    start, lst = F3.brick_lists(Nz, Nx, Ny, nodes)
    nbz, nbx = -(-Nz // TZ), -(-Nx // TX)
    assert len(start) == nbz * nbx * -(-Ny // TY) + 1 == 3 * 4 * 3 + 1 and start[0] == 0 and start[-1] == 400 and np.all(np.diff(start) >= 0)
    assert sorted(lst.tolist()) == list(range(400))
    for b in range(len(start) - 1):
        for q in lst[start[b]:start[b + 1]]:
            i, j, k = nodes[q] % Nz, nodes[q] // Nz % Nx, nodes[q] // Nz // Nx
            assert (i // TZ, j // TX, k // TY) == (b % nbz, b // nbz % nbx, b // nbz // nbx)
        assert np.all(np.diff(lst[start[b]:start[b + 1]]) > 0)
    s0, l0 = F3.brick_lists(Nz, Nx, Ny, np.zeros(0, np.int32))
    assert np.all(s0 == 0) and l0.size == 0
    for bad in (Nz * Nx * Ny, -1):
        with pytest.raises(_lib.QdasError, match="outside the grid"):
            F3.brick_lists(Nz, Nx, Ny, np.array([bad], np.int32))
    with pytest.raises(_lib.QdasError, match="no bricks"):
        F3.brick_lists(1 << 11, 1 << 10, 1 << 10, np.zeros(1, np.int32))


def _volume_system(nel=2, pitch=0.5e-3, Z=30, X=20, Y=16, fs=10e6):
    z, x, y = np.arange(Z) * H, (np.arange(X) - (X - 1) / 2) * H, (np.arange(Y) - (Y - 1) / 2) * H
    return UltrasoundSystem(Transducer.matrix(nel, pitch, FC), Sequence("FSA", c0=C0), Scan.cartesian(x, z, y), fs=fs), (z, x, y)


def test_plan_of_a_volume_against_hand_values():
    us, (z, x, y) = _volume_system()
    c = np.full((30, 20, 16), C0)
    wv = _burst(1 / 60e6)
    plan = us.fdtdSim(c, waveform=wv, wv_t0=-0.4e-6, wv_fs=60e6, plan_only=True, rx_impulse=np.ones(3), rx_t0=-0.05e-6, PML=6)
    assert (plan["ratio"], plan["fs_"], plan["P"], plan["Nz"], plan["Nx"], plan["Ny"]) == (6, 60e6, 6, 42, 32, 28)
    assert plan["txn0"] == -24 and plan["txne"] == -24 + len(wv) - 1
    T = 2 * np.sqrt((29 * H) ** 2 + (19 * H) ** 2 + (15 * H) ** 2) / C0
    assert plan["T"] == pytest.approx(T, rel=1e-12) and plan["Nt"] == 1 + int(np.floor((T + (len(wv) - 1) / 60e6) * 60e6 + 1e-9))
    assert plan["t0"] == pytest.approx(-24 / 60e6 - 0.05e-6, abs=1e-15)
    assert plan["rho"].shape == (30, 20, 16) and np.all(plan["rho"] == C0 / 1.5) and plan["rho_iso"] is None
    # 2 x 2 elements at +-0.25 mm in x and y, z = 0: x nodes at -0.95 + 0.1 k -> 7 (-0.25) and 12 (+0.25); y nodes at -0.75 + 0.1 k -> 5 and 10; x fastest
    siz, six, siy = plan["src_nodes"]
    assert siz.tolist() == [0] * 4 and six.tolist() == [7, 12, 7, 12] and siy.tolist() == [5, 5, 10, 10]
    assert all(np.array_equal(a, b) for a, b in zip(plan["sen_nodes"], plan["src_nodes"]))
    c2 = c.copy()
    c2[10:20] = 1600.0
    iso = us.fdtdSim(c2, None, isosub=True, rho0=1000.0, waveform=np.ones(3), wv_t0=0.0, wv_fs=60e6, plan_only=True)
    assert iso["rho_iso"].shape == (30, 20, 16) and iso["rho_iso"][15, 0, 0] == pytest.approx(937.5) and iso["ratio"] == 7


def test_the_dispatch_and_the_refusals_of_the_wrapper():
    us, (z, x, y) = _volume_system()
    kw = dict(waveform=np.ones(3), wv_t0=0.0, wv_fs=60e6, plan_only=True)
    c = np.full((30, 20, 16), C0)
    assert us.fdtdSim(c, **kw)["Ny"] == 16 + 40                                     # a volume no longer raises
    with pytest.raises(DasError, match="3-D"):                                     # the 2-D helper keeps its refusal: the volume route branches before it
        F.grid_spacing(np.arange(4) * H, np.arange(4) * H, np.arange(2) * H)
    # a 2-D grid plans exactly as before: none of the volume's keys, the 2-D default T
    us2 = UltrasoundSystem(Transducer.linear(4, 0.3e-3, FC), Sequence("FSA", c0=C0), Scan.cartesian(x, z), fs=10e6)
    plan = us2.fdtdSim(np.full((30, 20), C0), **kw)
    assert "Ny" not in plan and len(plan["src_nodes"]) == 2 and plan["T"] == pytest.approx(2 * np.hypot(29 * H, 19 * H) / C0, rel=1e-12)
    # a slab with a singleton x and a non-singleton y is not a volume: the 2-D route refuses it as before
    us1 = UltrasoundSystem(Transducer.linear(4, 0.3e-3, FC), Sequence("FSA", c0=C0), Scan.cartesian(x[:1], z, y), fs=10e6)
    with pytest.raises(DasError, match="3-D"):
        us1.fdtdSim(np.full((30, 1, 16), C0), **kw)
    for method in ("linear", "karray-direct", "karray-depend"):
        with pytest.raises(NotImplementedError):
            us.fdtdSim(c, ElemMapMethod=method, **kw)
    with pytest.raises(DasError, match="size"):
        us.fdtdSim(np.full((30, 20, 15), C0), **kw)
    with pytest.raises(DasError, match="size"):
        us.fdtdSim(c, np.full((30, 20), 1000.0), **kw)
    with pytest.raises(DasError, match="prec"):
        us.fdtdSim(c, prec="half", **kw)
    usq = UltrasoundSystem(us.tx, us.seq, Scan.cartesian(x, z, 2 * y), fs=10e6)                 # dy = 2 h
    with pytest.raises(DasError, match="uniform"):
        usq.fdtdSim(c, **kw)
    usd, _ = _volume_system(nel=4, pitch=0.04e-3)                                                 # a pitch below the grid's spacing
    with pytest.raises(DasError, match="not unique"):
        usd.fdtdSim(c, **kw)
    with pytest.raises(DasError, match="stability limit"):                                       # ratio = 1: c dt / h = 0.46 > 0.4488 (the 2-D limit would pass it)
        us.fdtdSim(np.full((30, 20, 16), 460.0), CFL_max=0.5, **kw)
    with pytest.raises(DasError, match="2 GiB"):
        us.fdtdSim(c, field=True, T=2e-3, **{**kw, "plan_only": False})


# ---------------------------------------------------------------------------------------------------------------- the ABI
def _struct_names(header, name, args=False):
    body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    if args:
        return [n.strip(" *") for decl in body.split(";") if decl.strip() for n in re.sub(r"^(const\s+)?\w+\s", "", decl.strip()).split(",")]
    return [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]


def test_descriptor_against_the_header():
    with open(os.path.join(ROOT, "include", "qdas.h")) as f:
        header = f.read()
    assert _struct_names(header, "qdas_fdtd3_desc") == [n for n, _ in _lib.Fdtd3Desc._fields_]
    assert C.sizeof(_lib.Fdtd3Desc) == 14 * 8 + 2 * 8 + 4 * 4 + 8
    assert tuple(_struct_names(header, "qdas_fdtd3_args", args=True)) == _lib.FDTD3_ARGS and C.sizeof(_lib.Fdtd3Args) == 8 * len(_lib.FDTD3_ARGS) == 8 * 29
    for n, v in (("TZ", _lib.FDTD3_TZ), ("TX", _lib.FDTD3_TX), ("TY", _lib.FDTD3_TY), ("ZERO", _lib.FDTD3_ZERO)):
        assert re.search(rf"#define QDAS_FDTD3_{n} {v}\b", header)
    for sym in ("qdas_fdtd3", "qdas_fdtd3_bricks", "qdas_fdtd3_brick_lists"):
        assert sym in _lib.SYMBOLS and hasattr(_lib.lib(), sym)
    L = _lib.lib()
    assert L.qdas_fdtd3.argtypes == [C.POINTER(_lib.Fdtd3Desc), C.POINTER(_lib.Fdtd3Args)]
    TZ, TX, TY = F3.BRICK
    assert L.qdas_fdtd3_bricks(64, 2 * TX, 2 * TY) == 4 and L.qdas_fdtd3_bricks(65, TX + 1, TY + 1) == 8 and L.qdas_fdtd3_bricks(1, 1, 1) == 1
    # the 2-D descriptor is untouched
    assert C.sizeof(_lib.FdtdDesc) == 12 * 8 + 2 * 8 + 4 * 4 + 8 and "Ny" not in [n for n, _ in _lib.FdtdDesc._fields_]


def _desc(**kw):
    d = _lib.Fdtd3Desc()
    base = dict(Nz=49, Nx=41, Ny=11, V=2, Nt=3, ld=49, pstride=49 * 41, vstride=49 * 41 * 11, M=1, Ts=2, N=1, rec_st=2, rec_sn=2, rec_sv=1, dt_h=0.3, inv_h=1e4,
                dtype=1, order=8, device=-1)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return d


def _args(**null):
    a = _lib.Fdtd3Args()
    for n in _lib.FDTD3_ARGS:
        setattr(a, n, None if null.get(n) else 0x1000)          # never dereferenced: every row below is refused on the host
    return a


def test_every_validation_row():
    L = _lib.lib()
    last = lambda: L.qdas_last_error().decode()
    call = lambda d, a: L.qdas_fdtd3(C.byref(d), C.byref(a) if a is not None else None)
    assert L.qdas_fdtd3(None, None) == 1 and "null descriptor" in last()
    big = 1 << 31
    rows = [(dict(dtype=2), 1, "dtype"), (dict(dtype=7), 1, "dtype"), (dict(Nz=0), 1, "at least one node"), (dict(Nx=0), 1, "at least one node"),
            (dict(Ny=0), 1, "at least one node"), (dict(ld=48), 1, "ld = 48"), (dict(pstride=49 * 41 - 1), 1, "pstride"), (dict(vstride=49 * 41 * 11 - 1), 1, "vstride"),
            (dict(dt_h=0.0), 1, "finite and positive"), (dict(dt_h=float("nan")), 1, "finite and positive"), (dict(inv_h=float("inf")), 1, "finite and positive"),
            (dict(inv_h=-1.0), 1, "finite and positive"), (dict(order=6), 2, "order 6"), (dict(order=0), 2, "order 0"), (dict(flags=2), 1, "unknown flags"),
            (dict(Nz=1 << 11, ld=1 << 11, Nx=1 << 10, Ny=1 << 10, pstride=1 << 21, vstride=big), 2, "nodes reach 2\\^31"),
            (dict(Nz=1 << 16, ld=1 << 16, Nx=1 << 15, Ny=1, pstride=big, vstride=big), 2, "nodes reach 2\\^31"),
            (dict(Nz=1, ld=1 << 39, Nx=1 << 30, pstride=100), 1, "pstride = 100 is less"),               # (Nx ld = 2^69 does not fit 64 bits: compared by division)
            (dict(Nz=1, ld=1, Nx=1, Ny=1 << 30, pstride=1 << 43, vstride=100), 1, "vstride = 100 is less"),
            (dict(Ny=big, vstride=49 * 41 * big), 2, "reaches 2\\^31"), (dict(Nx=big, pstride=49 * big, vstride=49 * 11 * big), 2, "reaches 2\\^31"),
            (dict(ld=1 << 40, pstride=41 << 40, vstride=11 * 41 << 40), 2, "reaches 2\\^40"), (dict(pstride=1 << 44, vstride=11 << 44), 2, "reaches 2\\^44"),
            (dict(vstride=1 << 46), 2, "2\\^46"), (dict(V=65536), 2, "65535"), (dict(M=big), 2, "2\\^31"), (dict(N=big), 2, "2\\^31"), (dict(Nt=1 << 40), 2, "2\\^40"),
            (dict(rec_sn=1 << 40), 2, "2\\^40")]
    for kw, code, msg in rows:
        assert call(_desc(**kw), _args()) == code and re.search(msg, last()), (kw, last())
    assert call(_desc(), None) == 1 and "null argument block" in last()
    for name in _lib.FDTD3_ARGS:
        rc = call(_desc(), _args(**{name: True}))
        assert rc == 1 and "null pointer" in last(), (name, last())
    # nothing to do: QDAS_OK before any pointer is looked at
    assert call(_desc(Nt=0), None) == 0 and call(_desc(V=0), None) == 0
    # but an empty call is still validated
    assert call(_desc(Nt=0, order=6), None) == 2 and call(_desc(V=0, ld=3), None) == 1


def test_the_stream_travels_in_the_descriptor_and_there_is_no_work_space():
    with open(os.path.join(ROOT, "include", "qdas.h")) as f:
        header = f.read()
    assert not [n for n in stream_entries(header) if "fdtd" in n]
    proto = re.search(r"\bint\s+qdas_fdtd3\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1)
    assert "stream" not in proto and "qdas_fdtd3_desc" in proto and proto.count(",") == 1
    assert "queue" in [n for n, _ in _lib.Fdtd3Desc._fields_]
    from tests.test_scratch_host import scratch_users
    for fn in ("fdtd3.hip", "fdtd3_core.h"):
        with open(os.path.join(ROOT, "qups_amd", "csrc", fn)) as f:
            src = f.read()
        code = re.sub(r"//[^\n]*", "", src)
        assert not scratch_users(src) and "hipMalloc" not in src and "Synchronize" not in src and "atomic" not in code and "hipGraph" not in code
    with open(os.path.join(ROOT, "qups_amd", "csrc", "fdtd3_core.h")) as f:
        core = f.read()
    assert "hip/" not in core, "the core has no HIP dependency"
    assert '#include "fdtd_core.h"' in core and not re.search(r"\b(T|inline \w+) (coef|dplus|dminus|pml_update)\s*\(", core), "the 2-D core's arithmetic is reused, not copied"
    with open(os.path.join(ROOT, "qups_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert " fdtd3.hip" in mk and " fdtd3_core.h" in mk
    with open(os.path.join(ROOT, "qups_amd", "csrc", "fdtd3.hip")) as f:
        assert len(re.findall(r"<<<", re.sub(r"//[^\n]*", "", f.read()))) == 2, "two launches per time step"


# ---------------------------------------------------------------------------------------------------------------- the device's core, on the host
@pytest.fixture(scope="module")
def core_exe(tmp_path_factory):
    """fdtd3_core.h under AddressSanitizer and UBSan in a stand-alone program: LDS blocks, windows, states, tables and the record are heap blocks of exactly
    their size"""
    exe = str(tmp_path_factory.mktemp("fd3") / "fdtd3_core_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "qups_amd", "csrc"), os.path.join(ROOT, "tests", "fdtd3_core_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_core(exe, tmp_path, c, rho, h, dt, P, R_, src, nrm, s, sen, Nt, double, ld_extra=0, ps_extra=0):
    """the program on the tables qups_amd/fdtd3.py makes: ``(rec Nt x N x V, states V x Nz x Nx x Ny as the restatement holds them)``"""
    tab = F3.prepare(c, rho, h, dt, P)
    Nz, Nx, Ny = tab["Nz"], tab["Nx"], tab["Ny"]
    s = np.asarray(s, np.float64)
    Ts, M, V = s.shape
    node = lambda q: (((np.asarray(q[2], np.int64) + P) * Nx + np.asarray(q[1], np.int64) + P) * Nz + np.asarray(q[0], np.int64) + P).astype(np.int32)
    src_node, sen_node = node(src), node(sen)
    N = sen_node.size
    nrm = np.asarray(nrm, np.float64).reshape(3, -1)
    cs = tab["c"].reshape(-1)[src_node] if M else np.zeros(0)
    ld = Nz + ld_extra
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        np.array([0 if double else 1, R_, Nz, Nx, Ny, V, Nt, ld, Nx * ld + ps_extra, M, Ts, N, 0, 0], np.int64).tofile(f)
        np.array([dt / h, 1.0 / h]).tofile(f)
        for k in ("c2", "rho", "dtrz", "dtrx", "dtry", "az", "azs", "ax", "axs", "ay", "ays"):
            np.ascontiguousarray(tab[k], np.float64).tofile(f)
        np.ascontiguousarray(s).tofile(f)
        for a in range(3):
            (nrm[a] * 2.0 * cs * dt / h).tofile(f)
        src_node.tofile(f)
        sen_node.tofile(f)
    r = subprocess.run([exe, inp, out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    raw = np.fromfile(out)
    rec = raw[:Nt * N * V].reshape(Nt, N, V)
    st = raw[Nt * N * V:].reshape(7, V, Ny, Nx, Nz).transpose(0, 1, 4, 3, 2)
    return rec, dict(zip(F3.STATES, st))


def check_core(got, r64, d32, double, what):
    rec, st = got
    worst = 0.0
    for name, g, want in [("rec", rec, r64[0])] + [(k, st[k], r64[1][k]) for k in F3.STATES]:
        assert g.shape == want.shape
        err = np.abs(g - want).max() / np.abs(want).max()
        tol = R3.tolerance(d32[name], double)
        worst = max(worst, err / tol)
        assert err <= tol, (what, name, err, tol)
    print(f"fdtd3 core {what}: largest err / tolerance {worst:.3f}")


@pytest.mark.parametrize("R_", [1, 2, 4])
@pytest.mark.parametrize("grid", R3.GRIDS, ids=lambda g: "x".join(str(v) for v in g))
def test_the_core_on_the_host_matches_the_restatement(core_exe, tmp_path, grid, R_):
    """the GPU list's grids, one pulse, every order, float32 and float64"""
    cs, r64, _, d32 = R3.parity_refs(*grid, R_, 1)
    for double in (False, True):
        got = run_core(core_exe, tmp_path, cs["c"], cs["rho"], cs["h"], cs["dt"], grid[3], R_, cs["src"], cs["nrm"], cs["s"], cs["sen"], cs["Nt"], double)
        check_core(got, r64, d32, double, f"{grid} R = {R_} {'f64' if double else 'f32'}")


def _small_case(Z, X, Y, P, R_, src, sen, Nt=30, V=2):
    c = R3.smooth_map(Z, X, Y, 1400.0, 1680.0, Z + X + Y)
    rho = R3.smooth_map(Z, X, Y, 900.0, 1100.0, Z * X * Y)
    dt = 0.3 * H / c.max()
    rng = np.random.default_rng(Z)
    M = len(src[0])
    s = rng.standard_normal((10, M, V))
    nrm = np.stack([np.linspace(1, -1, M), np.linspace(0.2, 1, M), np.linspace(-0.5, 0.7, M)])
    run = lambda dt_: R3.simulate(c, rho, H, dt, P, R_, src, nrm, s, sen, Nt, dt_)
    r64, r32 = run(np.float64), run(np.float32)
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max()) if b.size and np.abs(b).max() > 0 else 0.0
    d32 = {"rec": rel(r32[0], r64[0])}
    d32.update({k: rel(r32[1][k], r64[1][k]) for k in F3.STATES})
    return (c, rho, H, dt, P, R_, src, nrm, s, sen, Nt), r64, d32


@pytest.mark.parametrize("Z,X,Y,P,R_", [(9, 7, 5, 0, 4), (4, 4, 4, 0, 4), (1, 1, 1, 0, 4), (1, 3, 2, 0, 1), (2, 5, 3, 0, 2), (3, 2, 20, 0, 4), (70, 3, 2, 0, 4), (6, 5, 4, 3, 4)])
def test_the_core_over_broken_inputs(core_exe, tmp_path, Z, X, Y, P, R_):
    """index lists that point at the first and at the last node (of the whole array with P = 0), grids smaller than one brick, a one-node grid, extents
    below R, padded row and plane strides"""
    one = Z * X * Y == 1
    first_last = tuple(np.array([0] if one else [0, n - 1]) for n in (Z, X, Y))
    args, r64, d32 = _small_case(Z, X, Y, P, R_, first_last, first_last)
    for double in (False, True):
        got = run_core(core_exe, tmp_path, *args, double, ld_extra=3 if double else 0, ps_extra=5 if double else 0)
        check_core(got, r64, d32, double, f"{Z} x {X} x {Y} P = {P} R = {R_}")


def test_the_core_without_sources_or_sensors_or_steps(core_exe, tmp_path):
    none = (np.zeros(0, int),) * 3
    one = (np.array([3]), np.array([2]), np.array([1]))
    args, r64, _ = _small_case(9, 7, 5, 2, 4, one, none)
    rec, st = run_core(core_exe, tmp_path, *args, False)
    assert rec.size == 0 and np.abs(st["p"]).max() > 0
    args, r64, _ = _small_case(9, 7, 5, 2, 4, none, one)
    rec, st = run_core(core_exe, tmp_path, *args, False)
    assert np.all(rec == 0) and all(np.all(v == 0) for v in st.values())
    args, _, _ = _small_case(9, 7, 5, 2, 4, one, one, Nt=0)
    rec, st = run_core(core_exe, tmp_path, *args, True)
    assert rec.size == 0 and all(np.all(v == 0) for v in st.values())


def test_gateway_compiles_and_links():
    """mex/qdas_mex.c with the 'fdtd3' command against the fake MEX API of tests/fake_mex (the run itself needs a GPU: tests/test_mex_fdtd3.py)"""
    from tests import test_mex_fdtd3 as M
    exe = M.build_gateway()
    assert os.path.exists(exe)
