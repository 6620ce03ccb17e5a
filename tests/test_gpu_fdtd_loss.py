"""qdas_fdtd_lossy and its Python layer (``fdtd.fdtd(alpha=...)``, ``UltrasoundSystem.fdtdSim(alpha=...)``) on the device, against the numpy restatement
tests/fdtd_loss_ref.py.

TOLERANCE: the rule of tests/test_gpu_fdtd.py, calibrated by the restatement and never by the device.  For each case the restatement runs in float32 and in
float64, ``d32 = max|ref32 - ref64| / max|ref64|`` per output; the device's float32 result must lie within ``8 d32`` of ``ref64`` (floor 1e-6), its float64
result within ``8 d32 2^-29`` (floor 1e-13), relative to the output's own maximum: the record, the five final states and the memory variables ``e``.  Every
case prints ``fdtd loss ratio`` = err / tolerance and the largest so far.

CASES: the grids (37, 29, 6), (64, 64, 0), (3, 130, 4), (130, 3, 4) of tests/fdtd_ref.py x R in {1, 4} x L in {0 (Stokes), 1, 3, 4} x both precisions, with
V = 1 or 3 alternating over (grid, R, L): 64 of the 128 combinations, every grid, order, mechanism count and precision with both pulse counts.  The loss map of
a case (``fdtd_loss_ref.loss_case``) is 0 over part of the grid and strong elsewhere.

PHYSICS: the case of tests/test_fdtd_loss_host.py from the device's float32 record, inside the same bound (twice the float64 restatement's deviation)."""
import numpy as np
import pytest
import torch

from qups_amd import Scan, Sequence, Transducer, UltrasoundSystem, _lib
from qups_amd import fdtd as F
from tests import fdtd_loss_ref as LR
from tests import fdtd_ref as R
from tests import guards as GD
from tests import streams as ST
from tests.test_fdtd_loss_host import PHYS_DEV, PHYS_FREQS

pytestmark = pytest.mark.gpu

FILL_MS = 16
SEEN = {"ratio": 0.0}
NAMES = (*F.STATES, "e")
GRIDS = [(37, 29, 6), (64, 64, 0), (3, 130, 4), (130, 3, 4)]
CASES = [(g, R_, (1, 3)[(gi + ri + li) % 2], L, prec) for gi, g in enumerate(GRIDS) for ri, R_ in enumerate((1, 4)) for li, L in enumerate((0, 1, 3, 4))
         for prec in ("single", "double")]


def positions(cs, which):
    iz, ix = cs[which]
    return np.stack([cs["z"][iz], cs["x"][ix]])


def block(ls):
    return dict(mode="relax" if len(ls["g"]) else "stokes", g=ls["g"], E=ls["E"], kap=ls["kap"])


def run_case(cs, ls, R_, prec, monkeypatch=None, **kw):
    call = lambda: F.fdtd(cs["c"], cs["rho"], cs["z"], cs["x"], positions(cs, "src"), cs["nrm"], kw.pop("s", cs["s"]), positions(cs, "sen"), kw.pop("Nt", cs["Nt"]),
                          cs["dt"], PML=cs["P"], order=2 * R_, prec=prec, return_state=True, loss=None if ls is None else block(ls), **kw)
    if monkeypatch is None:
        out = call()
        torch.cuda.synchronize()
        return out
    with GD.guard_outputs(monkeypatch) as g:
        rec, st = call()
        assert g.check(rec, *st.values()) >= 6 + (1 if ls is not None and len(ls["g"]) else 0)       # the record, the five states and e, each between its bands
    return rec, st


def host(st, k):
    """a state as the restatement holds it: ``V x Z' x X'`` (``e``: ``V x L x Z' x X'``)"""
    return st[k].cpu().numpy().swapaxes(-1, -2)


def compare(rec, st, r64, d32, double, what):
    worst, bad = 0.0, []
    for name, got, want in [("rec", rec.cpu().numpy(), r64[0])] + [(k, host(st, k), r64[1][k]) for k in NAMES if k in st or r64[1][k].size]:
        assert got.shape == want.shape, (name, got.shape, want.shape)
        if not want.size:
            continue
        err = np.abs(got.astype(np.float64) - want).max() / np.abs(want).max()
        tol = R.tolerance(d32[name], double)
        worst = max(worst, err / tol)
        print(f"fdtd loss ratio {what} {name}: err {err:.3e}, d32 {d32[name]:.3e}, tol {tol:.3e}, ratio {err / tol:.3f}")
        if not err <= tol:
            bad.append((name, err, tol))
    SEEN["ratio"] = max(SEEN["ratio"], worst)
    print(f"fdtd loss ratio {what}: {worst:.3f} (largest so far {SEEN['ratio']:.3f})")
    assert not bad, (what, bad)


# ---------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("grid,R_,V,L,prec", CASES, ids=lambda v: "x".join(str(k) for k in v) if isinstance(v, tuple) else str(v))
def test_parity_with_the_restatement(grid, R_, V, L, prec, monkeypatch):
    cs, ls, r64, _, d32 = LR.parity_refs(*grid, R_, V, L)
    rec, st = run_case(cs, ls, R_, prec, monkeypatch)
    assert rec.dtype == (torch.float32 if prec == "single" else torch.float64) and tuple(rec.shape) == (cs["Nt"], len(cs["sen"][0]), V)
    assert ("e" in st) == (L > 0) and (L == 0 or tuple(st["e"].shape) == (V, L) + tuple(st["p"].shape[1:]))
    compare(rec, st, r64, d32, prec == "double", f"{grid} R = {R_} V = {V} L = {L} {prec}")


# ---------------------------------------------------------------------------------------------------------------- behaviour
@pytest.mark.parametrize("R_,prec", [(4, "single"), (4, "double"), (1, "single"), (2, "double"), (2, "single"), (1, "double")])
@pytest.mark.parametrize("L", [0, 3])
def test_a_zero_map_gives_the_bits_of_the_lossless_entry(L, R_, prec):
    """the lossy pass states the roundings of the lossless kernels (csrc/fdtd_core.h): every order and both precisions"""
    cs = R.parity_case(37, 29, 6, 3)
    ls = LR.loss_case(37, 29, L, cs["dt"])
    want, ws = run_case(cs, None, R_, prec)
    got, gs = run_case(cs, dict(ls, kap=np.zeros_like(ls["kap"])), R_, prec)
    for k in F.STATES:
        assert ST.same_bits(gs[k], ws[k]), k
    assert ST.same_bits(got, want)
    lossy, _ = run_case(cs, ls, R_, prec)
    assert not ST.same_bits(lossy, want)


@pytest.mark.parametrize("L", [0, 4])
def test_two_runs_give_the_same_bits(L):
    cs = R.parity_case(37, 29, 6, 3)
    ls = LR.loss_case(37, 29, L, cs["dt"])
    a, sa = run_case(cs, ls, 4, "single")
    b, sb = run_case(cs, ls, 4, "single")
    assert ST.same_bits(a, b) and all(ST.same_bits(sa[k], sb[k]) for k in sa)


def _prepared(cs, ls, order=8, **kw):
    return F.fdtd(cs["c"], cs["rho"], cs["z"], cs["x"], positions(cs, "src"), cs["nrm"], cs["s"], positions(cs, "sen"), cs["Nt"], cs["dt"], PML=cs["P"],
                  order=order, prepare_only=True, loss=block(ls), **kw)


def _fresh(meta, V, L, fill=0.0):
    st = {k: torch.full((V, meta["Nx"], meta["ld"]), fill, dtype=torch.float32, device="cuda") for k in F.STATES}
    st["e"] = torch.full((V, L, meta["Nx"], meta["ld"]), fill, dtype=torch.float32, device="cuda")
    return st, torch.empty((meta["Nt"], meta["N"], V), dtype=torch.float32, device="cuda")


def test_a_nan_in_one_pulses_memory_variables_stays_there():
    cs = R.parity_case(37, 29, 6, 3)
    ls = LR.loss_case(37, 29, 3, cs["dt"])
    meta, tb, s_dev = _prepared(cs, ls)
    out = []
    for poison in (False, True):
        st, rec = _fresh(meta, 3, 3)
        if poison:
            st["e"][1, 2] = float("nan")                          # the last mechanism of the middle pulse
        F.launch(meta, tb, st, s_dev, rec, 0)
        torch.cuda.synchronize()
        out.append((rec, st))
    (clean, sc), (bad, sb) = out
    for v in (0, 2):
        assert ST.same_bits(clean[:, :, v], bad[:, :, v]) and all(ST.same_bits(sc[k][v], sb[k][v]) for k in sc)
    assert torch.isnan(bad[:, :, 1]).any() and torch.isnan(sb["p"][1]).any() and torch.isnan(sb["e"][1, 2]).all()


def test_the_entry_clears_the_states_and_the_memory_variables_when_asked():
    """QDAS_FDTD_ZERO: NaN-filled states and ``e`` with a padded row stride give the bits of a start from zeroed ones, and the padding keeps its poison"""
    cs = R.parity_case(49, 33, 8, 2)
    ls = LR.loss_case(49, 33, 2, cs["dt"])
    meta, tb, s_dev = _prepared(cs, ls, ld=70)
    out = []
    for fill, flags in ((0.0, 0), (float("nan"), _lib.FDTD_ZERO)):
        st, rec = _fresh(meta, 2, 2, fill)
        F.launch(dict(meta, flags=flags), tb, st, s_dev, rec, 0)
        torch.cuda.synchronize()
        out.append((rec, st))
    assert ST.same_bits(out[0][0], out[1][0]) and all(ST.same_bits(out[0][1][k][..., :65], out[1][1][k][..., :65]) for k in NAMES)
    assert all(bool(torch.isnan(out[1][1][k][..., 65:]).all()) for k in NAMES)
    assert float(out[0][1]["e"].abs().max()) > 0


@pytest.mark.parametrize("prec,L", [("single", 4), ("double", 1), ("single", 0)])
def test_strided_states_with_guard_bands(prec, L, monkeypatch):
    """``ld = Nz + 7``: the record, the states and ``e`` sit between guard bands (``run_case`` checks them), and the row padding is never written"""
    grid = (37, 29, 6)
    cs, ls, r64, _, d32 = LR.parity_refs(*grid, 4, 3, L)
    rec, st = run_case(cs, ls, 4, prec, monkeypatch, ld=49 + 7)
    assert st["p"].stride(1) == 56 and (L == 0 or st["e"].stride() == (L * 41 * 56, 41 * 56, 56, 1))
    compare(rec, st, r64, d32, prec == "double", f"{grid} ld = Nz + 7 L = {L} {prec}")


def test_blocks_of_pulses_give_the_same_bits(monkeypatch):
    cs = R.parity_case(37, 29, 6, 3)
    ls = LR.loss_case(37, 29, 3, cs["dt"])
    a, sa = run_case(cs, ls, 4, "single", bsize=3)
    b, sb = run_case(cs, ls, 4, "single", bsize=1)
    c_, sc = run_case(cs, ls, 4, "single", bsize=2)
    assert ST.same_bits(a, b) and ST.same_bits(a, c_) and all(ST.same_bits(sa[k], sb[k]) and ST.same_bits(sa[k], sc[k]) for k in NAMES)
    # without return_state ONE set of 5 + L arrays of bsize pulses serves every block: the record, five states and e
    with GD.guard_outputs(monkeypatch) as g:
        rec = F.fdtd(cs["c"], cs["rho"], cs["z"], cs["x"], positions(cs, "src"), cs["nrm"], cs["s"], positions(cs, "sen"), cs["Nt"], cs["dt"], PML=6, order=8,
                     loss=block(ls), bsize=2)
        assert g.check(rec) == 1
    shapes = sorted(tuple(b_.inner.shape) for b_ in g.bufs)
    assert shapes == sorted([(cs["Nt"], 4, 3)] + [(2, 41, 49)] * 5 + [(2, 3, 41, 49)]), shapes
    assert ST.same_bits(rec, a)


def test_stream_delayed_producer_on_a_side_stream():
    from tests.test_gpu_raybackproject import own_stream
    grid, L = (37, 29, 6), 3
    cs, ls, r64, _, d32 = LR.parity_refs(*grid, 4, 3, L)
    meta, tb, s_dev = _prepared(cs, ls)
    names = list(tb)
    zeros, _ = _fresh(meta, 3, L)
    g = GD.Guard()

    def fn(s_, *rest):
        st = dict(zip(NAMES, rest[:6]))
        rec = g.empty((meta["Nt"], meta["N"], 3), torch.float32, "cuda")
        F.launch(meta, dict(zip(names, rest[6:])), st, s_, rec, 0, stream=side)
        return (rec,) + tuple(st[k] for k in NAMES)

    with own_stream() as side:                          # a stream that lives for this test only (tests/test_gpu_fdtd.py says why)
        outs, clones, early = ST.run_delayed(fn, [s_dev] + [zeros[k] for k in NAMES] + [tb[k] for k in names], side, FILL_MS)
    assert early, "the entry returned while the producer was still running: it synchronises nothing"
    g.check(outs[0], all_written=True)
    assert all(ST.same_bits(o, c_) for o, c_ in zip(outs, clones))
    compare(outs[0], dict(zip(NAMES, outs[1:])), r64, d32, False, "side stream")


def test_no_steps_and_no_pulses_launch_nothing():
    import ctypes as C
    L = _lib.lib()
    d = _lib.FdtdDesc()
    d.Nz, d.Nx, d.V, d.Nt, d.ld, d.vstride, d.dt_h, d.inv_h, d.dtype, d.order, d.device = 49, 41, 3, 0, 49, 49 * 41, 0.3, 1e4, 1, 8, -1
    q = _lib.FdtdLoss()
    q.mode, q.L = _lib.FDTD_LOSS_RELAX, 1
    q.g[0], q.E[0] = 1.0, 0.5
    assert L.qdas_fdtd_lossy(C.byref(d), None, C.byref(q)) == 0           # null pointers: a launch would have been refused or would fault
    d.Nt, d.V = 10, 0
    assert L.qdas_fdtd_lossy(C.byref(d), None, C.byref(q)) == 0
    cs = R.parity_case(37, 29, 6, 3)
    ls = LR.loss_case(37, 29, 2, cs["dt"])
    rec, st = run_case(cs, ls, 4, "single", Nt=0)
    assert tuple(rec.shape) == (0, 4, 3) and all(float(st[k].abs().max()) == 0.0 for k in NAMES)
    rec, st = run_case(cs, ls, 4, "single", s=np.zeros((R.TS, len(cs["src"][0]), 0)))
    assert tuple(rec.shape) == (cs["Nt"], 4, 0) and tuple(st["e"].shape) == (0, 2, 41, 49)


# ---------------------------------------------------------------------------------------------------------------- physics
_BASE = {}


def _physics_run(**kw):
    ps = LR.physics_setup()
    z, x = np.arange(ps["Z"]) * ps["h"], (np.arange(ps["X"]) - ps["X"] // 2) * ps["h"]
    c = np.full((ps["Z"], ps["X"]), LR.C0)
    pos = lambda pts: np.stack([z[pts[0]], x[pts[1]]])
    rec = F.fdtd(c, np.full_like(c, LR.RHO0), z, x, pos(ps["src"]), ps["nrm"], ps["s"], pos(ps["sen"]), ps["Nt"], ps["dt"], PML=ps["P"], order=2 * ps["R"], **kw)
    return ps, rec[:, :, 0].cpu().numpy()


@pytest.mark.parametrize("y,L", LR.YS)
def test_the_device_absorbs_by_the_power_law(y, L):
    if not _BASE:
        _BASE["rec"] = _physics_run()[1]
    ps, rec = _physics_run(alpha=LR.ALPHA_DB, alpha_power=y, alpha_band=LR.BAND, mechanisms=max(L, 1))
    got = LR.measured_alpha(rec, _BASE["rec"], ps["dt"], ps["d"], PHYS_FREQS)
    want = F.alpha_np(LR.ALPHA_DB, y) * (2 * np.pi * PHYS_FREQS) ** y
    dev = np.abs(got / want - 1).max()
    print(f"fdtd loss physics (device, float32) y = {y} L = {L}: alpha at 5 MHz {got[20]:.2f} Np/m (law {want[20]:.2f}), largest deviation {dev:.4%}, "
          f"bound {2 * PHYS_DEV[(y, L)]:.4%}")
    assert dev <= 2 * PHYS_DEV[(y, L)]


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_fdtdsim_with_absorption_through_das():
    """a density scatterer at 12 mm under 16 elements, FSA, with and without 0.5 dB/(MHz^1.1 cm): the DAS peak stays within one pixel and loses amplitude
    (0.5 x 2.5^1.1 = 1.37 dB/cm over 2.4 cm of path: about 3.3 dB)"""
    H, C0, FC, FS, SCAT = 1e-4, 1500.0, 2.5e6, 10e6, (120, 101)
    z, x = np.arange(170) * H, (np.arange(200) - 99.5) * H
    zi, xi = np.arange(10e-3, 14.01e-3, 0.05e-3), np.arange(-1.5e-3, 1.51e-3, 0.1e-3)
    us = UltrasoundSystem(Transducer.linear(16, 0.3e-3, FC), Sequence("FSA", c0=C0), Scan.cartesian(xi, zi), fs=FS)
    wt = np.arange(-48, 49) / 60e6
    kw = dict(waveform=np.sin(2 * np.pi * FC * wt) * np.exp(-(wt / 0.35e-6) ** 2), wv_t0=wt[0], wv_fs=60e6, c0=C0, rho0=1000.0, isosub=True)
    c = np.full((170, 200), C0)
    rho = np.full((170, 200), 1000.0)
    rho[SCAT] *= 2
    cgrd = Scan.cartesian(x, z)
    peaks = {}
    for name, extra in (("lossless", {}), ("lossy", dict(alpha=0.5, alpha_power=1.1))):
        chd = us.fdtdSim(c, rho, cgrd, **kw, **extra)
        b = us.DAS(chd.downsample(int(round(chd.fs / FS))).hilbert(), c0=C0).abs().reshape(len(zi), len(xi)).cpu().numpy()
        k = np.unravel_index(b.argmax(), b.shape)
        peaks[name] = (k, float(b[k]))
        print(f"fdtd loss end to end {name}: fs_ {chd.fs / 1e6:g} MHz, peak at pixel {tuple(int(v) for v in k)} (z {zi[k[0]] * 1e3:.2f} mm, x {xi[k[1]] * 1e3:.2f} mm), amplitude {b[k]:.4e}")
    (k0, a0), (k1, a1) = peaks["lossless"], peaks["lossy"]
    assert abs(k0[0] - k1[0]) <= 1 and abs(k0[1] - k1[1]) <= 1
    assert a1 < a0 and a1 > 0.3 * a0
    print(f"fdtd loss end to end: amplitude ratio {a1 / a0:.3f} ({20 * np.log10(a1 / a0):.2f} dB)")
