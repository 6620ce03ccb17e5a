"""qdas_fdtd and its Python layer (qups_amd/fdtd.py, UltrasoundSystem.fdtdSim) on the device, against the numpy restatement tests/fdtd_ref.py.

TOLERANCE, calibrated by the restatement and never by the device: for each case the restatement runs in float32 and in float64, and
``d32 = max|ref32 - ref64| / max|ref64|`` per output.  The device's float32 result must lie within ``8 d32`` of ``ref64`` (floor 1e-6), its float64 result
within ``8 d32 2^-29`` (floor 1e-13), relative to the output's own maximum: the record over all steps and each of the five final state arrays.  The factor 8
covers FMA contraction and another order of the 2R-term sums.  Every case prints ``fdtd ratio`` = err / tolerance; the largest over every case of this file on
one MI355X is 0.226 in float32 ((130, 3, 4), R = 1, V = 1) and 0.109 in float64.

GRIDS ``(Z, X, P)`` (tests/fdtd_ref.py GRIDS): the kernel's tile is 64 (z) x 16 (x) nodes of the extended grid ``(Z + 2P) x (X + 2P)``: 49 x 41 (no tile
multiple), 64 x 64 (exactly 1 x 4 tiles), 11 x 138 and 138 x 11 (thinner inside than the halo of R = 4), 65 x 49 (one node past a tile both ways).

END TO END.  32 elements at 0.3 mm pitch, FSA, fc = 2.5 MHz, c0 = 1500 m/s, h = 0.1 mm, a 170 x 200 grid; a horizontal layer of 1250 m/s in rows 30 .. 89
(6 mm) between the array and a density scatterer (rho x 2) at node (120, 101), constant impedance elsewhere, isosub.  Predicted depth error of DAS at c0:
6 mm (1500 / 1250 - 1) = 1.2 mm = 2.0 lambda.  The restatement on the CPU with 8 transmits (every fourth element; float32, a numpy DAS with straight-ray and
with layered-ray delays) gave the figures quoted in ``test_end_to_end_layer``'s docstring.

The entry takes its stream in the descriptor's ``queue`` field: the stream case is in this file."""
import ctypes as C

import numpy as np
import pytest
import torch

from qups_amd import ChannelData, DasError, Scan, Sequence, Transducer, UltrasoundSystem, _lib
from qups_amd import fdtd as F
from tests import fdtd_ref as R
from tests import guards as GD
from tests import streams as ST

pytestmark = pytest.mark.gpu

FILL_MS = 16
SEEN = {"ratio": 0.0}
NPT = {"single": np.float32, "double": np.float64}


def positions(cs, which):
    iz, ix = cs[which]
    return np.stack([cs["z"][iz], cs["x"][ix]])


def run_case(cs, R_, prec, monkeypatch=None, **kw):
    call = lambda: F.fdtd(cs["c"], cs["rho"], cs["z"], cs["x"], positions(cs, "src"), cs["nrm"], kw.pop("s", cs["s"]), positions(cs, "sen"), kw.pop("Nt", cs["Nt"]),
                          cs["dt"], PML=cs["P"], order=2 * R_, prec=prec, return_state=True, **kw)
    if monkeypatch is None:
        out = call()
        torch.cuda.synchronize()
        return out
    with GD.guard_outputs(monkeypatch) as g:
        rec, st = call()
        assert g.check(rec, *st.values()) >= 6                # the bands of every buffer; the record and the five states written by this call
    return rec, st


def compare(rec, st, r64, d32, double, what):
    worst = 0.0
    for name, got, want in [("rec", rec.cpu().numpy(), r64[0])] + [(k, st[k].cpu().numpy().transpose(0, 2, 1), r64[1][k]) for k in F.STATES]:
        assert got.shape == want.shape, (name, got.shape, want.shape)
        err = np.abs(got.astype(np.float64) - want).max() / np.abs(want).max()
        tol = R.tolerance(d32[name], double)
        worst = max(worst, err / tol)
        print(f"fdtd ratio {what} {name}: err {err:.3e}, d32 {d32[name]:.3e}, tol {tol:.3e}, ratio {err / tol:.3f}")
    SEEN["ratio"] = max(SEEN["ratio"], worst)
    print(f"fdtd ratio {what}: {worst:.3f} (largest so far {SEEN['ratio']:.3f})")
    for name, got, want in [("rec", rec.cpu().numpy(), r64[0])] + [(k, st[k].cpu().numpy().transpose(0, 2, 1), r64[1][k]) for k in F.STATES]:
        err = np.abs(got.astype(np.float64) - want).max() / np.abs(want).max()
        assert err <= R.tolerance(d32[name], double), (what, name, err, R.tolerance(d32[name], double))


# ---------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("prec", ["single", "double"])
@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("R_", [1, 2, 4])
@pytest.mark.parametrize("grid", R.GRIDS, ids=lambda g: "x".join(str(v) for v in g))
def test_parity_with_the_restatement(grid, R_, V, prec, monkeypatch):
    cs, r64, _, d32 = R.parity_refs(*grid, R_, V)
    rec, st = run_case(cs, R_, prec, monkeypatch)
    assert rec.dtype == (torch.float32 if prec == "single" else torch.float64) and tuple(rec.shape) == (cs["Nt"], len(cs["sen"][0]), V)
    compare(rec, st, r64, d32, prec == "double", f"{grid} R = {R_} V = {V} {prec}")


# ---------------------------------------------------------------------------------------------------------------- behaviour
def test_two_runs_give_the_same_bits():
    cs = R.parity_case(49, 33, 8, 3)
    a, sa = run_case(cs, 4, "single")
    b, sb = run_case(cs, 4, "single")
    assert ST.same_bits(a, b) and all(ST.same_bits(sa[k], sb[k]) for k in F.STATES)


def test_a_nan_in_one_pulse_stays_there():
    cs = R.parity_case(37, 29, 6, 3)
    clean, sc = run_case(cs, 4, "single")
    s = np.array(cs["s"])
    s[5, 1, 1] = np.nan
    bad, sb = run_case(cs, 4, "single", s=s)
    for v in (0, 2):
        assert ST.same_bits(clean[:, :, v], bad[:, :, v]) and all(ST.same_bits(sc[k][v], sb[k][v]) for k in F.STATES)
    assert torch.isnan(bad[:, :, 1]).any() and torch.isnan(sb["p"][1]).any()


def test_blocks_of_pulses_give_the_same_bits():
    cs = R.parity_case(37, 29, 6, 3)
    a, sa = run_case(cs, 2, "single", bsize=3)
    b, sb = run_case(cs, 2, "single", bsize=1)
    c_, _ = run_case(cs, 2, "single", bsize=2)
    assert ST.same_bits(a, b) and ST.same_bits(a, c_) and all(ST.same_bits(sa[k], sb[k]) for k in F.STATES)


def test_blocks_of_pulses_bound_the_state_memory(monkeypatch):
    """without ``return_state`` ONE set of five state arrays of ``bsize`` pulses serves every block: six allocations (the record and the five), whatever V"""
    cs = R.parity_case(37, 29, 6, 3)
    call = lambda **kw: F.fdtd(cs["c"], cs["rho"], cs["z"], cs["x"], positions(cs, "src"), cs["nrm"], cs["s"], positions(cs, "sen"), cs["Nt"], cs["dt"], PML=cs["P"],
                               order=4, **kw)
    want = call()
    for bsize, pulses in ((1, 1), (2, 2)):
        with GD.guard_outputs(monkeypatch) as g:
            rec = call(bsize=bsize)
            assert g.check(rec) == 1
        shapes = sorted(tuple(b.inner.shape) for b in g.bufs)
        assert shapes == sorted([(cs["Nt"], 4, 3)] + [(pulses, 41, 49)] * 5), shapes
        assert ST.same_bits(rec, want)


def test_the_entry_clears_the_states_when_asked():
    """QDAS_FDTD_ZERO: poisoned (NaN) state arrays with a padded row stride give the bits of a start from zeroed ones, and the padding keeps its poison"""
    cs = R.parity_case(49, 33, 8, 2)
    meta, tb, s_dev = F.fdtd(cs["c"], cs["rho"], cs["z"], cs["x"], positions(cs, "src"), cs["nrm"], cs["s"], positions(cs, "sen"), cs["Nt"], cs["dt"], PML=cs["P"],
                             order=8, prepare_only=True, ld=70)
    out = []
    for fill, flags in ((0.0, 0), (float("nan"), _lib.FDTD_ZERO)):
        st = {k: torch.full((2, meta["Nx"], meta["ld"]), fill, dtype=torch.float32, device="cuda") for k in F.STATES}
        rec = torch.empty((meta["Nt"], meta["N"], 2), dtype=torch.float32, device="cuda")
        F.launch(dict(meta, flags=flags), tb, st, s_dev, rec, 0)
        torch.cuda.synchronize()
        out.append((rec, st))
    assert ST.same_bits(out[0][0], out[1][0]) and all(ST.same_bits(out[0][1][k][:, :, :65], out[1][1][k][:, :, :65]) for k in F.STATES)
    assert all(bool(torch.isnan(out[1][1][k][:, :, 65:]).all()) for k in F.STATES)


@pytest.mark.parametrize("prec", ["single", "double"])
def test_strided_state_arrays(prec, monkeypatch):
    grid = (49, 33, 8)
    cs, r64, _, d32 = R.parity_refs(*grid, 4, 3)
    rec, st = run_case(cs, 4, prec, monkeypatch, ld=cs["c"].shape[0] + 2 * grid[2] + 7)
    assert st["p"].stride(1) == 65 + 7
    compare(rec, st, r64, d32, prec == "double", f"{grid} ld = Nz + 7 {prec}")


def test_no_steps_and_no_pulses_launch_nothing():
    L = _lib.lib()
    d = _lib.FdtdDesc()
    d.Nz, d.Nx, d.V, d.Nt, d.ld, d.vstride, d.dt_h, d.inv_h, d.dtype, d.order, d.device = 49, 41, 3, 0, 49, 49 * 41, 0.3, 1e4, 1, 8, -1
    assert L.qdas_fdtd(C.byref(d), None) == 0                     # null pointers: a launch would have been refused or would fault
    d.Nt, d.V = 10, 0
    assert L.qdas_fdtd(C.byref(d), None) == 0
    cs = R.parity_case(37, 29, 6, 3)
    rec, st = run_case(cs, 4, "single", Nt=0)
    assert tuple(rec.shape) == (0, 4, 3) and all(float(st[k].abs().max()) == 0.0 for k in F.STATES)
    rec, st = run_case(cs, 4, "single", s=np.zeros((R.TS, len(cs["src"][0]), 0)))
    assert tuple(rec.shape) == (cs["Nt"], 4, 0) and tuple(st["p"].shape) == (0, 41, 49)


def _node_system(cs, fs):
    """a system whose elements sit on the case's source nodes (normals along z) and whose scan is the case's grid"""
    iz, ix = cs["src"]
    pos = np.stack([cs["x"][ix], np.zeros(len(ix)), cs["z"][iz]])
    nrm = np.stack([np.zeros(len(ix)), np.zeros(len(ix)), np.ones(len(ix))])
    scan = Scan.cartesian(cs["x"], cs["z"])
    return UltrasoundSystem(Transducer(pos, nrm, 2.5e6), Sequence("FSA", c0=1500.0), scan, fs=fs)


def test_field_equals_the_restatements_snapshots():
    Z, X, P = 37, 29, 6
    cs = R.parity_case(Z, X, P, 1)
    us = _node_system(cs, 1.0 / cs["dt"])
    w = np.sin(2 * np.pi * np.arange(33) / 16.0) * np.hanning(33)
    kw = dict(waveform=w, wv_t0=0.0, wv_fs=1.0 / cs["dt"], PML=P, CFL_max=0.31, T=60 * cs["dt"])
    plan = us.fdtdSim(cs["c"], cs["rho"], plan_only=True, **kw)
    assert plan["ratio"] == 1 and plan["Nt"] == 93
    chd = us.fdtdSim(cs["c"], cs["rho"], field=True, **kw)
    M = len(cs["src"][0])
    assert tuple(chd.data.shape) == (plan["Nt"], Z * X, M) and chd.fs == 1.0 / cs["dt"] and chd.t0 == 0.0
    s, _, _ = F.tx_table(w, 0.0, 1.0 / cs["dt"], np.zeros((M, M)), np.eye(M), 1.0 / cs["dt"])
    nrm = np.stack([np.ones(M), np.zeros(M)])
    snaps = {}
    for dt_ in (np.float64, np.float32):
        snaps[dt_] = R.simulate(cs["c"], cs["rho"], cs["h"], cs["dt"], P, 4, cs["src"], nrm, s, ([], []), plan["Nt"], dt_, snapshots=True)[2]
    want = snaps[np.float64].reshape(plan["Nt"], Z * X, M)
    d32 = np.abs(snaps[np.float32] - snaps[np.float64]).max() / np.abs(want).max()
    err = np.abs(chd.data.cpu().numpy() - want).max() / np.abs(want).max()
    print(f"fdtd ratio field: err {err:.3e}, d32 {d32:.3e}, ratio {err / R.tolerance(d32, False):.3f}")
    assert err <= R.tolerance(d32, False)
    with pytest.raises(DasError, match="2 GiB"):
        us.fdtdSim(cs["c"], cs["rho"], field=True, **{**kw, "T": 0.02})


def test_receive_impulse_response_isosub_and_double():
    """the receive impulse response is a 'full' convolution along time with ``t0`` moved by its start; ``isosub`` is the difference of two runs; ``prec``"""
    Z, X, P = 37, 29, 6
    cs = R.parity_case(Z, X, P, 1)
    fs = 1.0 / cs["dt"]
    us = _node_system(cs, fs)
    w = np.sin(2 * np.pi * np.arange(33) / 16.0) * np.hanning(33)
    kw = dict(waveform=w, wv_t0=0.0, wv_fs=fs, PML=P, CFL_max=0.31, T=60 * cs["dt"], c0=1500.0, rho0=1000.0)
    plain = us.fdtdSim(cs["c"], cs["rho"], **kw)
    M = len(cs["src"][0])
    assert tuple(plain.data.shape) == (93, M, M) and plain.order == "TNM" and plain.data.dtype == torch.float32
    imp = np.array([0.5, 1.0, -0.25])
    conv = us.fdtdSim(cs["c"], cs["rho"], rx_impulse=imp, rx_t0=-cs["dt"], **kw)
    assert tuple(conv.data.shape) == (95, M, M) and conv.t0 == pytest.approx(plain.t0 - cs["dt"], abs=1e-18) and conv.fs == plain.fs
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
    grid = (49, 33, 8)
    cs, r64, _, d32 = R.parity_refs(*grid, 4, 3)
    meta, tb, s_dev = F.fdtd(cs["c"], cs["rho"], cs["z"], cs["x"], positions(cs, "src"), cs["nrm"], cs["s"], positions(cs, "sen"), cs["Nt"], cs["dt"], PML=cs["P"],
                             order=8, prec="single", prepare_only=True)
    names = list(tb)
    zeros = [torch.zeros((3, meta["Nx"], meta["ld"]), dtype=torch.float32, device="cuda") for _ in F.STATES]
    g = GD.Guard()

    def fn(s_, *rest):
        st = dict(zip(F.STATES, rest[:5]))
        rec = g.empty((meta["Nt"], meta["N"], 3), torch.float32, "cuda")
        F.launch(meta, dict(zip(names, rest[5:])), st, s_, rec, 0, stream=side)
        return (rec,) + tuple(st[k] for k in F.STATES)

    with own_stream() as side:                          # (not torch.cuda.Stream(): a pool stream lives on and moves the later files' streams to other hardware queues)
        outs, clones, early = ST.run_delayed(fn, [s_dev] + zeros + [tb[k] for k in names], side, FILL_MS)
    assert early, "the entry returned while the producer was still running: it synchronises nothing"
    g.check(outs[0], all_written=True)
    assert all(ST.same_bits(o, c_) for o, c_ in zip(outs, clones))
    compare(outs[0], dict(zip(F.STATES, outs[1:])), r64, d32, False, "side stream")


# ---------------------------------------------------------------------------------------------------------------- end to end
H, C0, FC, FS = 1e-4, 1500.0, 2.5e6, 10e6
LAM = C0 / FC
SCAT = (120, 101)


def _e2e_system():
    z, x = np.arange(170) * H, (np.arange(200) - 99.5) * H
    xdc = Transducer.linear(32, 0.3e-3, FC)
    cgrd = Scan.cartesian(x, z)
    zi, xi = np.arange(10e-3, 15.01e-3, 0.05e-3), np.arange(-1.5e-3, 1.51e-3, 0.1e-3)
    us = UltrasoundSystem(xdc, Sequence("FSA", c0=C0), Scan.cartesian(xi, zi), fs=FS)
    wt = np.arange(-48, 49) / 60e6
    w = np.sin(2 * np.pi * FC * wt) * np.exp(-(wt / 0.35e-6) ** 2)
    return us, cgrd, z, x, zi, xi, dict(waveform=w, wv_t0=wt[0], wv_fs=60e6, c0=C0, rho0=1000.0)


def _peak(b, zi, xi):
    a = b.abs().reshape(len(zi), len(xi)).cpu().numpy()
    k = np.unravel_index(a.argmax(), a.shape)
    return k, zi[k[0]], xi[k[1]]


def _analytic(chd, ratio):
    return chd.downsample(ratio).hilbert()


def test_end_to_end_layer():
    """fdtdSim -> downsample -> hilbert -> DAS at c0 and bfEikonal through the true map.  The restatement on the CPU with 8 transmits (float32, a numpy DAS
    with straight-ray and with layered-ray delays) gave: DAS peak at z = 13.15 mm (+1.92 lambda) and x = 0.20 mm, eikonal-equivalent peak at z = 11.95 mm
    (-0.08 lambda) and x = 0.10 mm; the scatterer is at z = 12.00 mm, x = 0.15 mm.  One MI355X with all 32 transmits: DAS 13.15 / 0.20, bfEikonal 11.85 / 0.10."""
    us, cgrd, z, x, zi, xi, kw = _e2e_system()
    c = np.full((170, 200), C0)
    c[30:90] = 1250.0
    rho = 1000.0 * C0 / c
    rho[SCAT] *= 2
    assert 6e-3 * (C0 / 1250.0 - 1) >= 1.5 * LAM
    chd = us.fdtdSim(c, rho, cgrd, isosub=True, **kw)
    assert tuple(chd.data.shape)[1:] == (32, 32) and chd.fs == 60e6 and 2000 < chd.data.shape[0] < 3000
    an = _analytic(chd, 6)
    _, zd, xd = _peak(us.DAS(an, c0=C0), zi, xi)
    _, ze, xe = _peak(us.bfEikonal(an, c.reshape(cgrd.size), cgrd), zi, xi)
    zs, xs = z[SCAT[0]], x[SCAT[1]]
    print(f"fdtd end to end: scatterer z {zs * 1e3:.2f} x {xs * 1e3:.2f} mm; DAS peak z {zd * 1e3:.2f} x {xd * 1e3:.2f}; bfEikonal peak z {ze * 1e3:.2f} x {xe * 1e3:.2f}")
    assert abs(ze - zs) <= LAM / 2 and abs(xe - xs) <= 0.3e-3
    assert abs(zd - zs) >= LAM


def test_end_to_end_homogeneous_twin_against_greens():
    """The same geometry with c = c0 everywhere: DAS on the fdtdSim record and on the greens record of the same scatterer, pixels of 0.05 mm in z and 0.1 mm
    in x.

    The leapfrog step is second order in time: its numerical phase velocity is c (1 + (c k dt)^2 / 24) and its group velocity c (1 + (c k dt)^2 / 8).  At 6
    points per wavelength (k h = 1.05) the envelope travels 0.86 % fast at c dt / h = 0.25 -- 0.10 mm of depth at z = 12 mm, two pixels, where the
    eighth-order space error is below 0.02 mm -- and 0.14 % fast at c dt / h = 0.1: 0.017 mm, a third of a pixel.  So:
      * at CFL_max = 0.1 the two peaks lie at the same pixel, within +-1 in z and x;
      * at the default CFL_max = 0.25 the fdtdSim peak lies TOWARDS THE ARRAY by the predicted 0.10 mm, give or take one pixel for each of the two peaks:
        1 to 4 pixels in z (0.05 .. 0.20 mm), within +-1 in x.
    The restatement on the CPU (4 transmits, float32) puts its DAS peak at z = 11.85 mm with CFL_max = 0.25 and at z = 12.00 mm, x = 0.20 mm with 0.1; one
    MI355X (32 transmits): 11.90 and 12.00 mm against 12.05 mm for greens.  The scatterer is at z = 12.00, x = 0.15 mm."""
    us, cgrd, z, x, zi, xi, kw = _e2e_system()
    c = np.full((170, 200), C0)
    rho = np.full((170, 200), 1000.0)
    rho[SCAT] *= 2
    # the same scatterer through greens: the two-way waveform of the FDTD chain is the transmit pulse (velocity source -> pressure -> density contrast)
    pos = np.array([[x[SCAT[1]]], [0.0], [z[SCAT[0]]]])
    g = us.greens(pos, np.ones(1), kw["waveform"], kw["wv_t0"], kw["wv_fs"], fs=FS, focus=False)
    gd = g.data if g.data.is_complex() else ChannelData(g.data, g.t0, g.fs, g.order).hilbert().data
    kg, zg, xg = _peak(us.DAS(ChannelData(gd, g.t0, g.fs, g.order), c0=C0), zi, xi)
    peaks = {}
    for cfl, fs_, ratio in ((0.1, 150e6, 15), (0.25, 60e6, 6)):
        chd = us.fdtdSim(c, rho, cgrd, isosub=True, CFL_max=cfl, **kw)
        assert chd.fs == fs_
        peaks[cfl] = _peak(us.DAS(_analytic(chd, ratio), c0=C0), zi, xi)
        kf, zf, xf = peaks[cfl]
        print(f"fdtd twin CFL_max = {cfl}: fdtdSim peak {tuple(int(v) for v in kf)} z {zf * 1e3:.2f} x {xf * 1e3:.2f}; greens peak {tuple(int(v) for v in kg)} z {zg * 1e3:.2f} x {xg * 1e3:.2f}")
    kf = peaks[0.1][0]
    assert abs(kf[0] - kg[0]) <= 1 and abs(kf[1] - kg[1]) <= 1
    kd = peaks[0.25][0]
    assert 1 <= kg[0] - kd[0] <= 4 and abs(kd[1] - kg[1]) <= 1


# ---------------------------------------------------------------------------------------------------------------- the wrapper's refusals on a device
def test_refusals():
    cs = R.parity_case(37, 29, 6, 1)
    with pytest.raises(DasError, match="stability"):
        F.fdtd(cs["c"], cs["rho"], cs["z"], cs["x"], positions(cs, "src"), cs["nrm"], cs["s"], positions(cs, "sen"), 5, 0.56 * cs["h"] / cs["c"].max(), PML=6)
    with pytest.raises(DasError, match="not unique"):
        F.fdtd(cs["c"], cs["rho"], cs["z"], cs["x"], positions(cs, "src")[:, [0, 0, 1, 2]], cs["nrm"], cs["s"], positions(cs, "sen"), 5, cs["dt"], PML=6)
