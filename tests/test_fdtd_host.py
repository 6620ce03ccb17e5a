"""qdas_fdtd without a GPU: the physics of the restatement tests/fdtd_ref.py (arrival times in a homogeneous and in a layered medium, the order of the
scheme, the PML, the rigid box), the wrapper arithmetic of qups_amd/fdtd.py and ``UltrasoundSystem.fdtdSim`` against hand values, the descriptor against the
header, the C entry's validation (``device = -1``: nothing reaches a HIP call), and the kernels' per-lane loops (``csrc/fdtd_core.h``) walked on the CPU by a
stand-alone program under AddressSanitizer and UBSan (tests/fdtd_core_host.cpp) against the restatement, within the GPU test's tolerance."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from qups_amd import DasError, Scan, Sequence, Transducer, UltrasoundSystem, _lib
from qups_amd import fdtd as F
from tests import fdtd_ref as R
from tests.test_streams_host import stream_entries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the physics of the restatement
H, C0, RHO0, FC = 1e-4, 1500.0, 1000.0, 2.5e6
DT = 0.25 * H / 1600.0


def _burst(dt):
    t = np.arange(0, 4.0 / FC, dt)
    tc = t.mean()
    return np.sin(2 * np.pi * FC * (t - tc)) * np.exp(-((t - tc) / (0.6 / FC)) ** 2)


@functools.lru_cache(maxsize=None)
def _lag(R_, layer):
    c = np.full((140, 81), C0)
    if layer:
        c[70:100] = 1600.0
    rec, _ = R.simulate(c, RHO0 * C0 / c, H, DT, 20, R_, ([2], [40]), [[1.0], [0.0]], _burst(DT)[:, None, None], ([52, 122], [40, 40]), 900)
    return R.xcorr_lag(rec[:, 0, 0], rec[:, 1, 0])


@pytest.mark.parametrize("layer,want", [(False, 298.67), (True, 290.67)])
def test_arrival_times_and_the_order_of_the_scheme(layer, want):
    """70 h / (c0 dt) = 298.67 samples between the sensors; 30 of the 70 rows at 1600 m/s: 290.67.  This restatement gives 297.88 / 289.85 at R = 4 and
    300.91 / 292.65 at R = 2 (6 points per wavelength: the fourth-order scheme is the more dispersive)."""
    l4, l2 = _lag(4, layer), _lag(2, layer)
    print(f"fdtd lag layer = {layer}: R = 4 {l4:.2f}, R = 2 {l2:.2f}, want {want}")
    assert abs(l4 - want) <= 1.5
    assert abs(l2 - want) > abs(l4 - want)


@functools.lru_cache(maxsize=None)
def _late(P):
    c = np.full((60, 41), C0)
    rec, _ = R.simulate(c, np.full_like(c, RHO0), H, DT, P, 4, ([30], [20]), [[1.0], [0.0]], _burst(DT)[:, None, None], ([30], [26]), 1500)
    return np.abs(rec[900:]).max(), np.abs(rec).max()


@pytest.mark.parametrize("P", [10, 20])
def test_the_pml_absorbs(P):
    """the late window (after every direct arrival) of a record in a small box: with a PML it falls below its rigid-box value"""
    late, peak = _late(P)
    late0, _ = _late(0)
    print(f"fdtd pml P = {P}: late / peak = {late / peak:.3e} ({20 * np.log10(late / peak):.1f} dB), rigid box {late0 / peak:.3e}")
    assert late < late0


def test_rigid_box_is_reproducible_and_stable_at_cfl_one_half():
    rng = np.random.default_rng(2)
    c = R.smooth_map(40, 36, 1400.0, 1600.0, 3)
    dt = 0.5 * H / c.max()
    assert 0.5 < R.limit(4) < 0.55
    s = rng.standard_normal((30, 2, 1))
    run = lambda: R.simulate(c, np.full_like(c, RHO0), H, dt, 0, 4, ([5, 30], [7, 20]), [[1.0, 0.0], [0.0, 1.0]], s, ([20], [18]), 2000)
    (ra, sa), (rb, sb) = run(), run()
    assert np.array_equal(ra, rb) and all(np.array_equal(sa[k], sb[k]) for k in sa)
    assert np.isfinite(ra).all() and all(np.isfinite(v).all() for v in sa.values())
    assert np.abs(ra[-500:]).max() < 50 * np.abs(ra[:500]).max(), "no growth: the energy of a lossless box stays"
    z, x = np.arange(40) * H, np.arange(36) * H
    with pytest.raises(DasError, match="stability limit"):
        F.fdtd(c, np.full_like(c, RHO0), z, x, np.zeros((2, 0)), np.zeros((2, 0)), np.zeros((1, 0, 1)), np.zeros((2, 0)), 1, 0.56 * H / c.max(), PML=0)
    with pytest.raises(DasError, match="stability limit"):
        F.time_step(10e6, 1160.0, 1e-4, CFL_max=0.58, order=8)                      # ratio = ceil(1.16 / 0.58) = 2: c dt / h = 0.58 > 0.5497
    assert F.time_step(10e6, 1160.0, 1e-4, CFL_max=0.58, order=4)[0] == 2           # 0.58 <= 0.606: inside the fourth-order limit


# ---------------------------------------------------------------------------------------------------------------- wrapper arithmetic
def test_time_step_against_hand_values():
    # dt_cfl = 0.25 * 1e-4 / 1500 = 16.67 ns; 1 / fs = 100 ns: ratio = ceil(6.0) = 6
    assert F.time_step(10e6, 1500.0, 1e-4, 0.25) == (6, 60e6, 1.0 / 60e6)
    assert F.time_step(10e6, 1540.0, 1e-4, 0.25)[0] == 7                            # 6.16 -> 7
    assert F.time_step(100e6, 1500.0, 1e-4, 0.25)[0] == 1                           # already fine enough: never below 1
    assert [round(F.stability_limit(r), 4) for r in (1, 2, 4)] == [0.7071, 0.6061, 0.5497]
    with pytest.raises(DasError, match="order"):
        F.time_step(10e6, 1500.0, 1e-4, 0.25, order=6)


def _system(nel=4, pitch=0.3e-3, Z=50, X=40, fs=10e6, seq=None):
    z, x = np.arange(Z) * H, (np.arange(X) - (X - 1) / 2) * H
    return UltrasoundSystem(Transducer.linear(nel, pitch, FC), seq or Sequence("FSA", c0=C0), Scan.cartesian(x, z), fs=fs)


def test_tx_table_record_length_and_t0_against_hand_values():
    fs_ = 60e6
    w = np.arange(1.0, 8.0)                                                          # 7 samples at 30 MHz from -0.1 us: tend = +0.1 us
    dl = np.array([[0.0, 0.05e-6], [0.02e-6, -0.03e-6]])                             # delays(seq, tx): del = -delays
    ap = np.array([[1.0, 0.5], [2.0, 1.0]])
    s, txn0, txne = F.tx_table(w, -0.1e-6, 30e6, dl, ap, fs_)
    assert txn0 == int(np.floor((-0.1e-6 - 0.05e-6) * fs_)) == -9 and txne == int(np.ceil((0.1e-6 + 0.03e-6) * fs_)) == 8
    assert s.shape == (18, 2, 2)
    # element 0, pulse 0 (no delay, apod 1): the waveform at t_n = (n - 9) / 60 MHz; its own samples fall on n = 3, 5, ..., 15
    assert np.allclose(s[3:16:2, 0, 0], w) and s[0, 0, 0] == pytest.approx(-0.0625)    # index -1.5: the cubic's last tap alone, u^2 (u - 1) / 2 at u = 1/2
    assert np.allclose(s[0:13:2, 0, 1], 0.5 * w)                                     # delays = +0.05 us: del = -3 samples, the waveform 3 samples earlier, apod 0.5
    us = _system()
    c = np.full((50, 40), C0)
    wv = _burst(1 / 60e6)
    plan = us.fdtdSim(c, waveform=wv, wv_t0=-0.4e-6, wv_fs=60e6, plan_only=True, rx_impulse=np.ones(3), rx_t0=-0.05e-6)
    assert (plan["ratio"], plan["fs_"], plan["P"], plan["Nz"], plan["Nx"]) == (6, 60e6, 20, 90, 80)
    assert plan["txn0"] == -24 and plan["txne"] == -24 + len(wv) - 1
    T = 2 * np.hypot(49 * H, 39 * H) / C0
    assert plan["T"] == pytest.approx(T, rel=1e-12) and plan["Nt"] == 1 + int(np.floor((T + (len(wv) - 1) / 60e6) * 60e6 + 1e-9))
    assert plan["t0"] == pytest.approx(-24 / 60e6 - 0.05e-6, abs=1e-15)
    assert np.array_equal(plan["rho"], np.full((50, 40), C0 / 1.5)), "rho = None: c0 / 1.5 everywhere"
    assert plan["rho_iso"] is None


def test_pml_size_rule():
    assert F.pml_size(20, 100, 100) == 20 and F.pml_size(0, 7, 9) == 0
    # Z + 2P, X + 2P for P = 10 .. 14 with Z = 100, X = 108: (120, 128) -> 5; (122, 130) -> 61; (124, 132) -> 31; (126, 134) -> 67; (128, 136) -> 17
    assert F.pml_size([10, 14], 100, 108) == 10
    # Z = X = 101: 121 -> 11, 123 -> 41, 125 -> 5, 127 -> 127, 129 -> 43
    assert F.pml_size([10, 14], 101, 101) == 12
    with pytest.raises(DasError):
        F.pml_size(-1, 10, 10)
    with pytest.raises(DasError):
        F.pml_size([5, 3], 10, 10)
    for bad in ([5], [5, 6, 7], []):
        with pytest.raises(DasError, match="range"):
            F.pml_size(bad, 10, 10)
    a, a_s = F.pml_factors(12, 4, 1500.0, 1e-4, 1e-8)
    assert np.all(a[4:8] == 1.0) and a[0] == a[11] == pytest.approx(np.exp(-2 * 1.5e7 * 1e-8 / 2)) and a[3] == a[8] == pytest.approx(np.exp(-2 * 1.5e7 * (1 / 4) ** 4 * 1e-8 / 2))
    assert a_s[3] == pytest.approx(np.exp(-2 * 1.5e7 * (0.5 / 4) ** 4 * 1e-8 / 2)) and np.all(a_s[4:7] == 1.0) and a_s[7] == pytest.approx(a_s[3])
    assert np.allclose(np.stack(F.pml_factors(12, 4, 1500.0, 1e-4, 1e-8)), np.stack(R.pml(12, 4, 1500.0, 1e-4, 1e-8)), rtol=1e-15)
    assert all(np.all(v == 1.0) for v in F.pml_factors(5, 0, 1500.0, 1e-4, 1e-8))


def test_nearest_nodes_and_the_duplicate_node_error():
    z, x = np.arange(5) * 1e-3, np.arange(-3, 4) * 1e-3
    iz, ix = F.nearest_nodes(z, x, np.array([[-2.9e-3, 0.4e-3, 3e-3], [0, 0, 0], [0.0, 1.6e-3, 9e-3]]))
    assert iz.tolist() == [0, 2, 4] and ix.tolist() == [0, 3, 6]
    iz, ix = F.nearest_nodes(z, x, np.array([[1.2e-3], [-1e-3]]))                   # two rows: (z, x)
    assert (int(iz[0]), int(ix[0])) == (1, 2)
    with pytest.raises(DasError, match="Elements are not unique; the Scan spacing or sizing may be too small."):
        F.nearest_nodes(z, x, np.array([[0.1e-3, 0.3e-3], [0, 0], [0.0, 0.0]]))
    us = _system(nel=8, pitch=0.04e-3)                                              # a pitch below the grid's spacing
    with pytest.raises(DasError, match="not unique"):
        us.fdtdSim(np.full((50, 40), C0), waveform=np.ones(3), wv_t0=0.0, wv_fs=60e6, plan_only=True)


def test_isosub_medium_and_the_refusals_of_the_wrapper():
    us = _system()
    c = np.full((50, 40), C0)
    c[20:30] = 1600.0
    kw = dict(waveform=np.ones(3), wv_t0=0.0, wv_fs=60e6, plan_only=True)
    plan = us.fdtdSim(c, None, isosub=True, rho0=1000.0, **kw)
    assert np.allclose(plan["rho_iso"], 1500.0 * 1000.0 / c) and plan["rho_iso"][25, 0] == pytest.approx(937.5)
    for method in ("linear", "karray-direct", "karray-depend"):
        with pytest.raises(NotImplementedError):
            us.fdtdSim(c, ElemMapMethod=method, **kw)
    with pytest.raises(DasError, match="3-D"):
        F.grid_spacing(np.arange(4) * H, np.arange(4) * H, np.arange(2) * H)
    with pytest.raises(DasError, match="uniform"):
        F.grid_spacing(np.arange(4) * H, np.arange(4) * 2 * H)
    with pytest.raises(DasError, match="uniform"):
        F.grid_spacing(np.array([0, 1, 2, 3.001]) * H, np.arange(4) * H)
    assert F.grid_spacing(np.array([0, 1, 2, 3.0000001]) * H, np.arange(4) * H) == pytest.approx(H, rel=1e-6)
    with pytest.raises(DasError, match="size"):
        us.fdtdSim(np.full((50, 41), C0), **kw)
    with pytest.raises(DasError, match="prec"):
        us.fdtdSim(c, prec="half", **kw)


def test_tile_lists_hold_every_point_exactly_once():
    assert (_lib.FDTD_TZ, _lib.FDTD_TX) == (R.TZ, R.TX) == F.TILE
    Nz, Nx = 138, 49
    rng = np.random.default_rng(1)
    nodes = rng.choice(Nz * Nx, 300, replace=False).astype(np.int32)
    nodes[:4] = [0, Nz * Nx - 1, 64 + 16 * Nz, 63 + 15 * Nz]
    start, lst = F.tile_lists(Nz, Nx, nodes)
    ntz = -(-Nz // R.TZ)
    assert len(start) == ntz * -(-Nx // R.TX) + 1 == 13 and start[0] == 0 and start[-1] == 300 and np.all(np.diff(start) >= 0)
    assert sorted(lst.tolist()) == list(range(300))
    for t in range(len(start) - 1):
        for k in lst[start[t]:start[t + 1]]:
            assert (nodes[k] % Nz) // R.TZ == t % ntz and (nodes[k] // Nz) // R.TX == t // ntz
        assert np.all(np.diff(lst[start[t]:start[t + 1]]) > 0)
    s0, l0 = F.tile_lists(Nz, Nx, np.zeros(0, np.int32))
    assert np.all(s0 == 0) and l0.size == 0
    with pytest.raises(_lib.QdasError, match="outside the grid"):
        F.tile_lists(Nz, Nx, np.array([Nz * Nx], np.int32))


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_descriptor_against_the_header():
    with open(os.path.join(ROOT, "include", "qdas.h")) as f:
        header = f.read()
    body = re.search(r"typedef struct qdas_fdtd_desc \{(.*?)\} qdas_fdtd_desc;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [n for n, _ in _lib.FdtdDesc._fields_]
    assert C.sizeof(_lib.FdtdDesc) == 12 * 8 + 2 * 8 + 4 * 4 + 8
    body = re.search(r"typedef struct qdas_fdtd_args \{(.*?)\} qdas_fdtd_args;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in re.sub(r"^(const\s+)?\w+\s", "", decl.strip()).split(",")]
    assert tuple(names) == _lib.FDTD_ARGS and C.sizeof(_lib.FdtdArgs) == 8 * len(_lib.FDTD_ARGS)
    assert re.search(r"#define QDAS_FDTD_TZ 64\b", header) and re.search(r"#define QDAS_FDTD_TX 16\b", header)
    for sym in ("qdas_fdtd", "qdas_fdtd_tiles", "qdas_fdtd_tile_lists"):
        assert sym in _lib.SYMBOLS and hasattr(_lib.lib(), sym)
    L = _lib.lib()
    assert L.qdas_fdtd.argtypes == [C.POINTER(_lib.FdtdDesc), C.POINTER(_lib.FdtdArgs)]
    assert L.qdas_fdtd_tiles(138, 49) == 12 and L.qdas_fdtd_tiles(64, 64) == 4 and L.qdas_fdtd_tiles(65, 17) == 4


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


def test_every_validation_row():
    L = _lib.lib()
    last = lambda: L.qdas_last_error().decode()
    call = lambda d, a: L.qdas_fdtd(C.byref(d), C.byref(a) if a is not None else None)
    assert L.qdas_fdtd(None, None) == 1 and "null descriptor" in last()
    rows = [(dict(dtype=2), 1, "dtype"), (dict(dtype=7), 1, "dtype"), (dict(Nz=0), 1, "at least one node"), (dict(Nx=0), 1, "at least one node"),
            (dict(ld=48), 1, "ld = 48"), (dict(vstride=49 * 41 - 1), 1, "vstride"), (dict(dt_h=0.0), 1, "finite and positive"),
            (dict(dt_h=float("nan")), 1, "finite and positive"), (dict(inv_h=float("inf")), 1, "finite and positive"), (dict(inv_h=-1.0), 1, "finite and positive"),
            (dict(order=6), 2, "order 6"), (dict(order=0), 2, "order 0"), (dict(Nz=1 << 16, ld=1 << 16, Nx=1 << 15, vstride=1 << 31), 2, "reach 2\\^31"),
            (dict(Nz=1, ld=1 << 39, Nx=1 << 30, vstride=100), 1, "vstride = 100 is less"),                 # (Nx ld = 2^69 does not fit 64 bits: compared by division)
            (dict(Nx=1 << 31, vstride=49 << 31), 2, "reaches 2\\^31"), (dict(ld=1 << 40, vstride=41 << 40), 2, "reaches 2\\^40"), (dict(flags=2), 1, "unknown flags"),
            (dict(V=65536), 2, "65535"), (dict(M=1 << 31), 2, "2\\^31"), (dict(Nt=1 << 40), 2, "2\\^40")]
    for kw, code, msg in rows:
        assert call(_desc(**kw), _args()) == code and re.search(msg, last()), (kw, last())
    assert call(_desc(), None) == 1 and "null argument block" in last()
    for name in _lib.FDTD_ARGS:
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
    proto = re.search(r"\bint\s+qdas_fdtd\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1)
    assert "stream" not in proto and "qdas_fdtd_desc" in proto and proto.count(",") == 1
    assert "queue" in [n for n, _ in _lib.FdtdDesc._fields_]
    from tests import test_gpu_fdtd as G
    assert callable(G.test_stream_delayed_producer_on_a_side_stream)
    from tests.test_scratch_host import scratch_users
    for fn in ("fdtd.hip", "fdtd_core.h"):
        with open(os.path.join(ROOT, "qups_amd", "csrc", fn)) as f:
            src = f.read()
        code = re.sub(r"//[^\n]*", "", src)
        assert not scratch_users(src) and "hipMalloc" not in src and "Synchronize" not in src and "atomic" not in code and "hipGraph" not in code
    with open(os.path.join(ROOT, "qups_amd", "csrc", "fdtd_core.h")) as f:
        assert "hip/" not in f.read(), "the core has no HIP dependency"
    with open(os.path.join(ROOT, "qups_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert " fdtd.hip" in mk and " fdtd_core.h" in mk
    with open(os.path.join(ROOT, "qups_amd", "csrc", "fdtd.hip")) as f:
        assert len(re.findall(r"<<<", re.sub(r"//[^\n]*", "", f.read()))) == 2, "two launches per time step"


# ---------------------------------------------------------------------------------------------------------------- the device's core, on the host
@pytest.fixture(scope="module")
def core_exe(tmp_path_factory):
    """fdtd_core.h under AddressSanitizer and UBSan in a stand-alone program: LDS blocks, states, tables and the record are heap blocks of exactly their size"""
    exe = str(tmp_path_factory.mktemp("fd") / "fdtd_core_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "qups_amd", "csrc"), os.path.join(ROOT, "tests", "fdtd_core_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_core(exe, tmp_path, c, rho, h, dt, P, R_, src, nrm, s, sen, Nt, double, ld_extra=0):
    """the program on the tables qups_amd/fdtd.py makes: ``(rec Nt x N x V, states V x Nz x Nx as the restatement holds them)``"""
    tab = F.prepare(c, rho, h, dt, P)
    Nz, Nx = tab["Nz"], tab["Nx"]
    s = np.asarray(s, np.float64)
    Ts, M, V = s.shape
    src_node = ((np.asarray(src[1], np.int64) + P) * Nz + np.asarray(src[0], np.int64) + P).astype(np.int32)
    sen_node = ((np.asarray(sen[1], np.int64) + P) * Nz + np.asarray(sen[0], np.int64) + P).astype(np.int32)
    N = sen_node.size
    nrm = np.asarray(nrm, np.float64).reshape(2, -1)
    cs = tab["c"].reshape(-1)[src_node] if M else np.zeros(0)
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        np.array([0 if double else 1, R_, Nz, Nx, V, Nt, Nz + ld_extra, M, Ts, N, 0, 0], np.int64).tofile(f)
        np.array([dt / h, 1.0 / h]).tofile(f)
        for k in ("c2", "rho", "dtrz", "dtrx", "az", "azs", "ax", "axs"):
            np.ascontiguousarray(tab[k], np.float64).tofile(f)
        np.ascontiguousarray(s).tofile(f)
        (nrm[0] * 2.0 * cs * dt / h).tofile(f)
        (nrm[1] * 2.0 * cs * dt / h).tofile(f)
        src_node.tofile(f)
        sen_node.tofile(f)
    r = subprocess.run([exe, inp, out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    raw = np.fromfile(out)
    rec = raw[:Nt * N * V].reshape(Nt, N, V)
    st = raw[Nt * N * V:].reshape(5, V, Nx, Nz).transpose(0, 1, 3, 2)
    return rec, dict(zip(F.STATES, st))


def check_core(got, r64, d32, double, what):
    rec, st = got
    worst = 0.0
    for name, g, want in [("rec", rec, r64[0])] + [(k, st[k], r64[1][k]) for k in F.STATES]:
        assert g.shape == want.shape
        err = np.abs(g - want).max() / np.abs(want).max()
        tol = R.tolerance(d32[name], double)
        worst = max(worst, err / tol)
        assert err <= tol, (what, name, err, tol)
    print(f"fdtd core {what}: largest err / tolerance {worst:.3f}")


@pytest.mark.parametrize("R_", [1, 2, 4])
@pytest.mark.parametrize("grid", R.GRIDS, ids=lambda g: "x".join(str(v) for v in g))
def test_the_core_on_the_host_matches_the_restatement(core_exe, tmp_path, grid, R_):
    """the GPU list's grids, V = 3; float32 for every grid and order, float64 for R = 4"""
    cs, r64, _, d32 = R.parity_refs(*grid, R_, 3)
    for double in ((False, True) if R_ == 4 else (False,)):
        got = run_core(core_exe, tmp_path, cs["c"], cs["rho"], cs["h"], cs["dt"], grid[2], R_, cs["src"], cs["nrm"], cs["s"], cs["sen"], cs["Nt"], double)
        check_core(got, r64, d32, double, f"{grid} R = {R_} {'f64' if double else 'f32'}")


def _small_case(Z, X, P, R_, src, sen, Nt=40, V=2, ld_extra=0):
    c = R.smooth_map(Z, X, 1400.0, 1680.0, Z + X)
    rho = R.smooth_map(Z, X, 900.0, 1100.0, Z * X)
    dt = 0.3 * H / c.max()
    rng = np.random.default_rng(Z)
    s = rng.standard_normal((10, len(src[0]), V))
    nrm = np.stack([np.linspace(1, -1, len(src[0])), np.linspace(0.2, 1, len(src[0]))])
    run = lambda dt_: R.simulate(c, rho, H, dt, P, R_, src, nrm, s, sen, Nt, dt_)
    r64, r32 = run(np.float64), run(np.float32)
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max()) if b.size and np.abs(b).max() > 0 else 0.0
    d32 = {"rec": rel(r32[0], r64[0])}
    d32.update({k: rel(r32[1][k], r64[1][k]) for k in F.STATES})
    return (c, rho, H, dt, P, R_, src, nrm, s, sen, Nt), r64, d32


@pytest.mark.parametrize("Z,X,P,R_", [(9, 7, 0, 4), (4, 4, 0, 4), (4, 30, 0, 4), (2, 5, 0, 2), (1, 3, 0, 1), (20, 5, 3, 4), (70, 20, 0, 4)])
def test_the_core_over_broken_inputs(core_exe, tmp_path, Z, X, P, R_):
    """index lists that point at the first and at the last node (of the whole array with P = 0), grids smaller than one tile, Nz = R, a padded row stride"""
    first_last = (np.array([0, Z - 1]), np.array([0, X - 1]))
    args, r64, d32 = _small_case(Z, X, P, R_, first_last, first_last)
    for double in (False, True):
        got = run_core(core_exe, tmp_path, *args, double, ld_extra=3 if double else 0)
        check_core(got, r64, d32, double, f"{Z} x {X} P = {P} R = {R_}")


def test_the_core_without_sources_or_sensors_or_steps(core_exe, tmp_path):
    none = (np.zeros(0, int), np.zeros(0, int))
    one = (np.array([3]), np.array([2]))
    args, r64, _ = _small_case(9, 7, 2, 4, one, none)
    rec, st = run_core(core_exe, tmp_path, *args, False)
    assert rec.size == 0 and np.abs(st["p"]).max() > 0
    args, r64, _ = _small_case(9, 7, 2, 4, none, one)
    rec, st = run_core(core_exe, tmp_path, *args, False)
    assert np.all(rec == 0) and all(np.all(v == 0) for v in st.values())
    args, _, _ = _small_case(9, 7, 2, 4, one, one, Nt=0)
    rec, st = run_core(core_exe, tmp_path, *args, True)
    assert rec.size == 0 and all(np.all(v == 0) for v in st.values())


def test_gateway_compiles_and_links():
    """mex/qdas_mex.c with the 'fdtd' command against the fake MEX API of tests/fake_mex (the run itself needs a GPU: tests/test_mex_fdtd.py)"""
    from tests import test_mex_fdtd as M
    exe = M.build_gateway()
    assert os.path.exists(exe)
