"""qdas_fdtd3 and its Python layer (qups_amd/fdtd3.py, UltrasoundSystem.fdtdSim on a volume) on the device, against the numpy restatement tests/fdtd3_ref.py.

TOLERANCE: the rule of tests/test_gpu_fdtd.py (``fdtd_ref.tolerance``), calibrated by the restatement and never by the device: for each case the restatement
runs in float32 and in float64, and ``d32 = max|ref32 - ref64| / max|ref64|`` per output.  The device's float32 result must lie within ``8 d32`` of ``ref64``
(floor 1e-6), its float64 result within ``8 d32 2^-29`` (floor 1e-13), relative to the output's own maximum: the record over all steps and each of the seven
final state arrays.  Every case prints ``fdtd3 ratio`` = err / tolerance; the largest over every case of this file on one MI355X is 0.424 in float32 and
0.306 in float64.

GRIDS ``(Z, X, Y, P)`` (tests/fdtd3_ref.py GRIDS, made from the header's brick 64 x TX x TY over the extended grid): (a) no extent a brick multiple, several
bricks in x and y; (b) exactly 64 x 2 TX x 2 TY without a PML; (c), (d), (e) 11 nodes (3 + 2 x 4, thinner than the halo of R = 4) along z, x, y in turn, the
other two one node past a brick edge; (f) every extent one node past a brick edge.

END TO END.  4 x 4 elements at 0.8 mm pitch, FSA, fc = 2.5 MHz, c0 = 1500 m/s, h = 0.1 mm, a 101 x 41 x 41 volume, PML 10; a horizontal layer of 1250 m/s in
rows 20 .. 69 (5 mm) between the array and a density scatterer (rho x 2) at node (80, 20, 20), constant impedance elsewhere, isosub.  Predicted depth error of
DAS at c0: 5 mm (1500 / 1250 - 1) = 1.0 mm = 1.67 lambda.  The restatement's prediction is quoted in ``test_end_to_end_layer``'s docstring.

The entry takes its stream in the descriptor's ``queue`` field: the stream case is in this file."""
import ctypes as C

import numpy as np
import pytest
import torch

from qups_amd import DasError, Scan, Sequence, Transducer, UltrasoundSystem, _lib
from qups_amd import fdtd as F
from qups_amd import fdtd3 as F3
from tests import fdtd3_ref as R3
from tests import guards as GD
from tests import streams as ST

pytestmark = pytest.mark.gpu

FILL_MS = 16
SEEN = {"single": 0.0, "double": 0.0}
GRID_IDS = [f"{n}-" + "x".join(str(v) for v in g) for n, g in zip("abcdef", R3.GRIDS)]


def positions(cs, which):
    iz, ix, iy = cs[which]
    return np.stack([cs["x"][ix], cs["y"][iy], cs["z"][iz]])


def run_case(cs, R_, prec, monkeypatch=None, **kw):
    call = lambda: F3.fdtd3(cs["c"], cs["rho"], cs["z"], cs["x"], cs["y"], positions(cs, "src"), cs["nrm"], kw.pop("s", cs["s"]), positions(cs, "sen"),
                            kw.pop("Nt", cs["Nt"]), cs["dt"], PML=cs["P"], order=2 * R_, prec=prec, return_state=True, **kw)
    if monkeypatch is None:
        out = call()
        torch.cuda.synchronize()
        return out
    with GD.guard_outputs(monkeypatch) as g:
        rec, st = call()
        assert g.check(rec, *st.values()) >= 8                # the bands of every buffer; the record and the seven states written by this call
    return rec, st


def _pairs(rec, st, r64):
    """(name, device array, reference array) with the device's ``V x Ny x Nx x Nz`` states turned to the restatement's ``V x Nz x Nx x Ny``"""
    return [("rec", rec.cpu().numpy(), r64[0])] + [(k, st[k].cpu().numpy().transpose(0, 3, 2, 1), r64[1][k]) for k in F3.STATES]


def compare(rec, st, r64, d32, double, what):
    worst, prec = 0.0, "double" if double else "single"
    rows = []
    for name, got, want in _pairs(rec, st, r64):
        assert got.shape == want.shape, (name, got.shape, want.shape)
        err = np.abs(got.astype(np.float64) - want).max() / np.abs(want).max()
        tol = R3.tolerance(d32[name], double)
        rows.append((name, err, tol))
        worst = max(worst, err / tol)
        print(f"fdtd3 ratio {what} {name}: err {err:.3e}, d32 {d32[name]:.3e}, tol {tol:.3e}, ratio {err / tol:.3f}")
    SEEN[prec] = max(SEEN[prec], worst)
    print(f"fdtd3 ratio {what}: {worst:.3f} (largest so far in {prec} {SEEN[prec]:.3f})")
    for name, err, tol in rows:
        assert err <= tol, (what, name, err, tol)


# ---------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("prec", ["single", "double"])
@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("R_", [1, 2, 4])
@pytest.mark.parametrize("grid", R3.GRIDS, ids=GRID_IDS)
def test_parity_with_the_restatement(grid, R_, V, prec, monkeypatch):
    cs, r64, _, d32 = R3.parity_refs(*grid, R_, V)
    rec, st = run_case(cs, R_, prec, monkeypatch)
    assert rec.dtype == (torch.float32 if prec == "single" else torch.float64) and tuple(rec.shape) == (cs["Nt"], len(cs["sen"][0]), V)
    compare(rec, st, r64, d32, prec == "double", f"{grid} R = {R_} V = {V} {prec}")


@pytest.mark.parametrize("prec", ["single", "double"])
def test_axis_swap_on_the_device(prec):
    """case (a) and its x <-> y transpose: x runs through LDS, y through the register window, so an index slip in either shows here.  Both lie within the
    tolerance of the one reference, and of each other."""
    grid, R_ = R3.GRIDS[0], 4
    cs, r64, _, d32 = R3.parity_refs(*grid, R_, 3)
    rec_a, st_a = run_case(cs, R_, prec)
    rec_b, st_b = run_case(R3.swap_xy(cs), R_, prec)
    back = {"p": "p", "uz": "uz", "ux": "uy", "uy": "ux", "rz": "rz", "rx": "ry", "ry": "rx"}
    st_b = {k: st_b[back[k]].permute(0, 2, 1, 3) for k in F3.STATES}         # V x Nx x Ny x Nz of the swapped run -> V x Ny x Nx x Nz of the original
    compare(rec_b, st_b, r64, d32, prec == "double", f"{grid} swapped R = {R_} {prec}")
    for name, a, b in [("rec", rec_a, rec_b)] + [(k, st_a[k], st_b[k]) for k in F3.STATES]:
        err = float((a.double() - b.double()).abs().max() / a.double().abs().max())
        assert err <= R3.tolerance(d32[name], prec == "double"), (name, err)


# ---------------------------------------------------------------------------------------------------------------- behaviour
def test_two_runs_give_the_same_bits():
    cs = R3.parity_case(*R3.GRIDS[5], 3)
    a, sa = run_case(cs, 4, "single")
    b, sb = run_case(cs, 4, "single")
    assert ST.same_bits(a, b) and all(ST.same_bits(sa[k], sb[k]) for k in F3.STATES)


def test_a_nan_in_one_pulse_stays_there():
    cs = R3.parity_case(*R3.GRIDS[0], 3)
    clean, sc = run_case(cs, 4, "single")
    s = np.array(cs["s"])
    s[5, 1, 1] = np.nan
    bad, sb = run_case(cs, 4, "single", s=s)
    for v in (0, 2):
        assert ST.same_bits(clean[:, :, v], bad[:, :, v]) and all(ST.same_bits(sc[k][v], sb[k][v]) for k in F3.STATES)
    assert torch.isnan(bad[:, :, 1]).any() and torch.isnan(sb["p"][1]).any()


def test_blocks_of_pulses_give_the_same_bits():
    cs = R3.parity_case(*R3.GRIDS[0], 3)
    a, sa = run_case(cs, 2, "single", bsize=3)
    b, sb = run_case(cs, 2, "single", bsize=1)
    c_, _ = run_case(cs, 2, "single", bsize=2)
    assert ST.same_bits(a, b) and ST.same_bits(a, c_) and all(ST.same_bits(sa[k], sb[k]) for k in F3.STATES)


def test_blocks_of_pulses_bound_the_state_memory(monkeypatch):
    """without ``return_state`` ONE set of seven state arrays of ``bsize`` pulses serves every block: eight allocations (the record and the seven), whatever V"""
    Z, X, Y, P = R3.GRIDS[0]
    cs = R3.parity_case(Z, X, Y, P, 3)
    call = lambda **kw: F3.fdtd3(cs["c"], cs["rho"], cs["z"], cs["x"], cs["y"], positions(cs, "src"), cs["nrm"], cs["s"], positions(cs, "sen"), cs["Nt"], cs["dt"],
                                 PML=P, order=4, **kw)
    want = call()
    N = len(cs["sen"][0])
    for bsize, pulses in ((1, 1), (2, 2)):
        with GD.guard_outputs(monkeypatch) as g:
            rec = call(bsize=bsize)
            assert g.check(rec) == 1
        shapes = sorted(tuple(b.inner.shape) for b in g.bufs)
        assert shapes == sorted([(cs["Nt"], N, 3)] + [(pulses, Y + 2 * P, X + 2 * P, Z + 2 * P)] * 7), shapes
        assert ST.same_bits(rec, want)


def test_the_entry_clears_the_states_when_asked():
    """QDAS_FDTD3_ZERO: poisoned (NaN) state arrays with padded row and plane strides give the bits of a start from zeroed ones, and the padding keeps its
    poison; a padded row stride alone takes the other branch of the clearing"""
    cs = R3.parity_case(*R3.GRIDS[5], 2)
    for ld_extra, ps_extra in ((5, 9), (5, 0), (0, 0)):
        Nz = cs["c"].shape[0] + 2 * cs["P"]
        Nx = cs["c"].shape[1] + 2 * cs["P"]
        ld = Nz + ld_extra
        meta, tb, s_dev = F3.fdtd3(cs["c"], cs["rho"], cs["z"], cs["x"], cs["y"], positions(cs, "src"), cs["nrm"], cs["s"], positions(cs, "sen"), cs["Nt"], cs["dt"],
                                   PML=cs["P"], order=8, prepare_only=True, ld=ld, pstride=Nx * ld + ps_extra)
        out = []
        for fill, flags in ((0.0, 0), (float("nan"), _lib.FDTD3_ZERO)):
            raw = {k: torch.full((2, meta["Ny"], meta["pstride"]), fill, dtype=torch.float32, device="cuda") for k in F3.STATES}
            st = {k: raw[k].as_strided((2, meta["Ny"], Nx, ld), (meta["Ny"] * meta["pstride"], meta["pstride"], ld, 1)) for k in F3.STATES}
            rec = torch.empty((meta["Nt"], meta["N"], 2), dtype=torch.float32, device="cuda")
            F3.launch(dict(meta, flags=flags), tb, st, s_dev, rec, 0)
            torch.cuda.synchronize()
            out.append((rec, st, raw))
        assert ST.same_bits(out[0][0], out[1][0]) and all(ST.same_bits(out[0][1][k][..., :Nz].contiguous(), out[1][1][k][..., :Nz].contiguous()) for k in F3.STATES)
        assert float(out[0][0].abs().max()) > 0
        if ld_extra:
            assert all(bool(torch.isnan(out[1][1][k][..., Nz:]).all()) for k in F3.STATES)
        if ps_extra:
            assert all(bool(torch.isnan(out[1][2][k][:, :, Nx * ld:]).all()) for k in F3.STATES)


@pytest.mark.parametrize("prec", ["single", "double"])
def test_strided_state_arrays(prec, monkeypatch):
    grid = R3.GRIDS[5]
    cs, r64, _, d32 = R3.parity_refs(*grid, 4, 3)
    Nz, Nx = grid[0] + 2 * grid[3], grid[1] + 2 * grid[3]
    rec, st = run_case(cs, 4, prec, monkeypatch, ld=Nz + 7, pstride=Nx * (Nz + 7) + 11)
    assert st["p"].stride(2) == Nz + 7 and st["p"].stride(1) == Nx * (Nz + 7) + 11
    compare(rec, st, r64, d32, prec == "double", f"{grid} ld = Nz + 7, pstride = Nx ld + 11 {prec}")


def test_no_steps_and_no_pulses_launch_nothing():
    L = _lib.lib()
    d = _lib.Fdtd3Desc()
    d.Nz, d.Nx, d.Ny, d.V, d.Nt, d.ld, d.pstride, d.vstride, d.dt_h, d.inv_h, d.dtype, d.order, d.device = 49, 41, 11, 3, 0, 49, 49 * 41, 49 * 41 * 11, 0.3, 1e4, 1, 8, -1
    assert L.qdas_fdtd3(C.byref(d), None) == 0                    # null pointers: a launch would have been refused or would fault
    d.Nt, d.V = 10, 0
    assert L.qdas_fdtd3(C.byref(d), None) == 0
    Z, X, Y, P = R3.GRIDS[0]
    cs = R3.parity_case(Z, X, Y, P, 3)
    N = len(cs["sen"][0])
    rec, st = run_case(cs, 4, "single", Nt=0)
    assert tuple(rec.shape) == (0, N, 3) and all(float(st[k].abs().max()) == 0.0 for k in F3.STATES)
    rec, st = run_case(cs, 4, "single", s=np.zeros((R3.TS, len(cs["src"][0]), 0)))
    assert tuple(rec.shape) == (cs["Nt"], N, 0) and tuple(st["p"].shape) == (0, Y + 2 * P, X + 2 * P, Z + 2 * P)


def _node_system(cs, fs):
    """a system whose elements sit on the case's source nodes (normals along z) and whose scan is the case's grid"""
    iz, ix, iy = cs["src"]
    pos = np.stack([cs["x"][ix], cs["y"][iy], cs["z"][iz]])
    nrm = np.stack([np.zeros(len(ix)), np.zeros(len(ix)), np.ones(len(ix))])
    scan = Scan.cartesian(cs["x"], cs["z"], cs["y"])
    return UltrasoundSystem(Transducer(pos, nrm, 2.5e6), Sequence("FSA", c0=1500.0), scan, fs=fs)


def test_field_equals_the_restatements_snapshots():
    Z, X, Y, P = R3.GRIDS[5]
    cs = R3.parity_case(Z, X, Y, P, 1)
    us = _node_system(cs, 1.0 / cs["dt"])
    w = np.sin(2 * np.pi * np.arange(33) / 16.0) * np.hanning(33)
    kw = dict(waveform=w, wv_t0=0.0, wv_fs=1.0 / cs["dt"], PML=P, CFL_max=0.31, T=40 * cs["dt"])
    plan = us.fdtdSim(cs["c"], cs["rho"], plan_only=True, **kw)
    assert plan["ratio"] == 1 and plan["Nt"] == 73
    chd = us.fdtdSim(cs["c"], cs["rho"], field=True, **kw)
    M = len(cs["src"][0])
    assert tuple(chd.data.shape) == (plan["Nt"], Z * X * Y, M) and chd.fs == 1.0 / cs["dt"] and chd.t0 == 0.0
    s, _, _ = F.tx_table(w, 0.0, 1.0 / cs["dt"], np.zeros((M, M)), np.eye(M), 1.0 / cs["dt"])
    nrm = np.stack([np.ones(M), np.zeros(M), np.zeros(M)])
    none = (np.zeros(0, int),) * 3
    snaps = {}
    for dt_ in (np.float64, np.float32):
        snaps[dt_] = R3.simulate(cs["c"], cs["rho"], cs["h"], cs["dt"], P, 4, cs["src"], nrm, s, none, plan["Nt"], dt_, snapshots=True)[2]
    want = snaps[np.float64].reshape(plan["Nt"], Z * X * Y, M)                 # the nodes in C order of (Z, X, Y)
    d32 = np.abs(snaps[np.float32] - snaps[np.float64]).max() / np.abs(want).max()
    err = np.abs(chd.data.cpu().numpy() - want).max() / np.abs(want).max()
    print(f"fdtd3 ratio field: err {err:.3e}, d32 {d32:.3e}, ratio {err / R3.tolerance(d32, False):.3f}")
    assert err <= R3.tolerance(d32, False)
    with pytest.raises(DasError, match="2 GiB"):
        us.fdtdSim(cs["c"], cs["rho"], field=True, **{**kw, "T": 0.05})


def test_receive_impulse_response_isosub_and_double():
    """the receive impulse response is a 'full' convolution along time with ``t0`` moved by its start; ``isosub`` is the difference of two runs; ``prec``"""
    Z, X, Y, P = R3.GRIDS[5]
    cs = R3.parity_case(Z, X, Y, P, 1)
    fs = 1.0 / cs["dt"]
    us = _node_system(cs, fs)
    w = np.sin(2 * np.pi * np.arange(33) / 16.0) * np.hanning(33)
    kw = dict(waveform=w, wv_t0=0.0, wv_fs=fs, PML=P, CFL_max=0.31, T=40 * cs["dt"], c0=1500.0, rho0=1000.0)
    plain = us.fdtdSim(cs["c"], cs["rho"], **kw)
    M = len(cs["src"][0])
    assert tuple(plain.data.shape) == (73, M, M) and plain.order == "TNM" and plain.data.dtype == torch.float32
    imp = np.array([0.5, 1.0, -0.25])
    conv = us.fdtdSim(cs["c"], cs["rho"], rx_impulse=imp, rx_t0=-cs["dt"], **kw)
    assert tuple(conv.data.shape) == (75, M, M) and conv.t0 == pytest.approx(plain.t0 - cs["dt"], abs=1e-18) and conv.fs == plain.fs
    x = plain.data.cpu().numpy().astype(np.float64)
    want = np.apply_along_axis(lambda v: np.convolve(v, imp), 0, x)
    assert np.abs(conv.data.cpu().numpy() - want).max() <= 1e-5 * np.abs(want).max()
    iso = us.fdtdSim(cs["c"], cs["rho"], isosub=True, **kw)
    twin = us.fdtdSim(cs["c"], 1500.0 * 1000.0 / cs["c"], **kw)
    assert ST.same_bits(iso.data, plain.data - twin.data)
    dbl = us.fdtdSim(cs["c"], cs["rho"], prec="double", **kw)
    assert dbl.data.dtype == torch.float64 and float((dbl.data - plain.data).abs().max()) <= 1e-4 * float(dbl.data.abs().max())


# ---------------------------------------------------------------------------------------------------------------- the stream
def test_stream_delayed_producer_on_a_side_stream():
    from tests.test_gpu_raybackproject import own_stream
    grid = R3.GRIDS[0]
    cs, r64, _, d32 = R3.parity_refs(*grid, 4, 3)
    meta, tb, s_dev = F3.fdtd3(cs["c"], cs["rho"], cs["z"], cs["x"], cs["y"], positions(cs, "src"), cs["nrm"], cs["s"], positions(cs, "sen"), cs["Nt"], cs["dt"],
                               PML=cs["P"], order=8, prec="single", prepare_only=True)
    names = list(tb)
    zeros = [torch.zeros((3, meta["Ny"], meta["Nx"], meta["ld"]), dtype=torch.float32, device="cuda") for _ in F3.STATES]
    g = GD.Guard()
    ns = len(F3.STATES)

    def fn(s_, *rest):
        st = dict(zip(F3.STATES, rest[:ns]))
        rec = g.empty((meta["Nt"], meta["N"], 3), torch.float32, "cuda")
        F3.launch(meta, dict(zip(names, rest[ns:])), st, s_, rec, 0, stream=side)
        return (rec,) + tuple(st[k] for k in F3.STATES)

    with own_stream() as side:                          # (not torch.cuda.Stream(): a pool stream lives on and moves the later files' streams to other hardware queues)
        outs, clones, early = ST.run_delayed(fn, [s_dev] + zeros + [tb[k] for k in names], side, FILL_MS)
    assert early, "the entry returned while the producer was still running: it synchronises nothing"
    g.check(outs[0], all_written=True)
    assert all(ST.same_bits(o, c_) for o, c_ in zip(outs, clones))
    compare(outs[0], dict(zip(F3.STATES, outs[1:])), r64, d32, False, "side stream")


# ---------------------------------------------------------------------------------------------------------------- end to end
H, C0, FC, FS = 1e-4, 1500.0, 2.5e6, 10e6
LAM = C0 / FC
SCAT = (80, 20, 20)
LAYER = (20, 70)


def _e2e_system():
    z, x, y = np.arange(101) * H, (np.arange(41) - 20) * H, (np.arange(41) - 20) * H
    xdc = Transducer.matrix(4, 0.8e-3, FC)
    cgrd = Scan.cartesian(x, z, y)
    zi, xi, yi = np.arange(6.5e-3, 9.501e-3, 0.05e-3), np.arange(-1e-3, 1.01e-3, 0.25e-3), np.arange(-1e-3, 1.01e-3, 0.25e-3)
    us = UltrasoundSystem(xdc, Sequence("FSA", c0=C0), Scan.cartesian(xi, zi, yi), fs=FS)
    wt = np.arange(-48, 49) / 60e6
    w = np.sin(2 * np.pi * FC * wt) * np.exp(-(wt / 0.35e-6) ** 2)
    return us, cgrd, (z, x, y), (zi, xi, yi), dict(waveform=w, wv_t0=wt[0], wv_fs=60e6, c0=C0, rho0=1000.0, PML=10)


def _peak(b, grid):
    a = b.abs().reshape(tuple(len(g) for g in grid)).cpu().numpy()
    k = np.unravel_index(a.argmax(), a.shape)
    return tuple(float(g[i]) for g, i in zip(grid, k))


def test_end_to_end_layer():
    """fdtdSim on a volume -> downsample -> hilbert -> DAS at c0 and bfEikonal through the true volume map, on a small volume scan around the scatterer
    (0.05 mm in z, 0.25 mm in x and y).  The restatement on the CPU with 4 transmits (elements 0, 6, 8, 15; float32, a numpy DAS with straight-ray delays at c0 and
    with Fermat delays through the three layers) gave: DAS peak at z = 8.95 mm (+1.58 lambda; predicted +1.67), x = y = 0; layered-ray peak at z = 8.00 mm,
    x = y = 0; the scatterer is at z = 8.00 mm, x = y = 0.  With 4 x 4 elements the lateral main lobe is wide -- the pixels 0.25 mm beside the peak reach 0.84
    to 0.89 of it in both images -- so the lateral assertion is one pixel.  One MI355X with all 16 transmits: DAS 8.95 / 0 / 0, bfEikonal 7.90 / 0 / 0
    (-0.17 lambda: the multistencil eikonal's own error through the two interfaces)."""
    us, cgrd, (z, x, y), grid, kw = _e2e_system()
    c = np.full((101, 41, 41), C0)
    c[LAYER[0]:LAYER[1]] = 1250.0
    rho = 1000.0 * C0 / c
    rho[SCAT] *= 2
    L = (LAYER[1] - LAYER[0]) * H
    assert L >= 4.5e-3 and L * (C0 / 1250.0 - 1) >= 1.5 * LAM
    chd = us.fdtdSim(c, rho, cgrd, isosub=True, **kw)
    T = 2 * np.sqrt(10e-3 ** 2 + 4e-3 ** 2 + 4e-3 ** 2) / C0
    assert tuple(chd.data.shape) == (1 + int(np.floor((T + 96 / 60e6) * 60e6 + 1e-9)), 16, 16) and chd.fs == 60e6
    assert chd.t0 == pytest.approx(-48 / 60e6, abs=1e-15)
    an = chd.downsample(6).hilbert()
    zd, xd, yd = _peak(us.DAS(an, c0=C0), grid)
    ze, xe, ye = _peak(us.bfEikonal(an, c, cgrd), grid)
    zs, xs, ys = z[SCAT[0]], x[SCAT[1]], y[SCAT[2]]
    mm = lambda *v: " ".join(f"{1e3 * q:.2f}" for q in v)
    print(f"fdtd3 end to end (z x y, mm): scatterer {mm(zs, xs, ys)}; DAS peak {mm(zd, xd, yd)}; bfEikonal peak {mm(ze, xe, ye)}")
    assert abs(ze - zs) <= LAM / 2 and abs(xe - xs) <= 0.25e-3 + 1e-9 and abs(ye - ys) <= 0.25e-3 + 1e-9
    assert zd - zs >= LAM and abs(xd - xs) <= 0.25e-3 + 1e-9 and abs(yd - ys) <= 0.25e-3 + 1e-9


# ---------------------------------------------------------------------------------------------------------------- the wrapper's refusals on a device
def test_refusals():
    cs = R3.parity_case(*R3.GRIDS[0], 1)
    args = lambda src, dt: (cs["c"], cs["rho"], cs["z"], cs["x"], cs["y"], src, cs["nrm"], cs["s"], positions(cs, "sen"), 5, dt)
    with pytest.raises(DasError, match="stability"):
        F3.fdtd3(*args(positions(cs, "src"), 0.46 * cs["h"] / cs["c"].max()), PML=3)
    with pytest.raises(DasError, match="not unique"):
        F3.fdtd3(*args(positions(cs, "src")[:, [0, 0, 1, 2]], cs["dt"]), PML=3)
    with pytest.raises(DasError, match="uniform"):
        F3.fdtd3(cs["c"], cs["rho"], cs["z"], cs["x"], 2 * cs["y"], positions(cs, "src"), cs["nrm"], cs["s"], positions(cs, "sen"), 5, cs["dt"], PML=3)
