"""qdas_fdtd_nonlinear and its Python layer (``fdtd.fdtd(BoA=...)``, ``UltrasoundSystem.fdtdSim(BoA=...)``) on the device, against the numpy restatement
tests/fdtd_nl_ref.py.

TOLERANCE: the rule of tests/test_gpu_fdtd.py, calibrated by the restatement and never by the device.  For each case the restatement runs in float32 and in
float64, ``d32 = max|ref32 - ref64| / max|ref64|`` per output; the device's float32 result must lie within ``8 d32`` of ``ref64`` (floor 1e-6), its float64
result within ``8 d32 2^-29`` (floor 1e-13), relative to the output's own maximum: the record, the five final states and the memory variables ``e``.  Every
case prints ``fdtd nl ratio`` = err / tolerance and the largest so far.

CASES: the grids (37, 29, 6), (64, 64, 0), (3, 130, 4), (130, 3, 4) of tests/fdtd_ref.py x R in {1, 2, 4} x V in {1, 3} x {no absorption, Stokes, L = 3} x
both precisions, driven hard (``fdtd_nl_ref.nl_case``: ``max|u| / c`` near 4e-3, B/A between 0 and 10): tests/test_fdtd_nl_host.py holds that every one of
them differs from its linear run by more than 100 x the tolerance.

PHYSICS: the Fubini case of tests/test_fdtd_nl_host.py from the device's float32 record, inside the same bounds (twice the float64 restatement's deviations).

QUADRATIC SCALING.  Four pulses ``+A, -A, +2A, -2A`` of the (37, 29, 6) case in one call, ``2A`` the amplitude of the parity cases.  Without ``BoA`` the sums
``rec(+A) + rec(-A)`` are exactly zero (the linear scheme is odd in its sources, in floating point too).  With it the sum at ``2A`` is 4 x the sum at ``A`` up
to the next order: the float64 restatement shows ``max|S(2A) - 4 S(A)| / max|4 S(A)|`` = 2.59e-4 (``QUAD_DEV``, measured once; the float32 restatement
2.35e-4, and ``S(A)`` is 3.6e-3 of the record); the device must stay within twice that.

END TO END (``fdtd_nl_ref.e2e_setup``): a 2.5 MHz plane wave from 16 elements into B/A = 6 with 0.5 dB/(MHz^1.01 cm) on a 0.05 mm grid, a density scatterer at
12 mm, isosub; a pulse-inversion pair -> half sum (harmonic) and half difference (fundamental) -> hilbert -> DAS at the solver's rate.  The float64
restatement on the CPU with a numpy DAS (linear interpolation at 140 MHz) gave the figures in ``test_tissue_harmonic_image_through_das``'s docstring."""
import numpy as np
import pytest
import torch

from qups_amd import ChannelData, _lib
from qups_amd import fdtd as F
from tests import fdtd_loss_ref as LR
from tests import fdtd_nl_ref as NR
from tests import fdtd_ref as R
from tests import guards as GD
from tests import streams as ST
from tests.test_fdtd_nl_host import PHYS_DEV, VARIANTS, check_fubini

pytestmark = pytest.mark.gpu

FILL_MS = 16
SEEN = {"ratio": 0.0}
NAMES = (*F.STATES, "e")
GRIDS = [(37, 29, 6), (64, 64, 0), (3, 130, 4), (130, 3, 4)]
CASES = [(g, R_, V, L, prec) for g in GRIDS for R_ in (1, 2, 4) for V in (1, 3) for L in NR.LOSSES for prec in ("single", "double")]
QUAD_DEV = 2.59e-4                  # measured on the float64 restatement (the module's docstring)


def positions(cs, which):
    iz, ix = cs[which]
    return np.stack([cs["z"][iz], cs["x"][ix]])


def block(ls):
    return None if ls is None else dict(mode="relax" if len(ls["g"]) else "stokes", g=ls["g"], E=ls["E"], kap=ls["kap"])


def run_case(cs, ls, R_, prec, monkeypatch=None, BoA="case", **kw):
    BoA = cs["BoA"] if isinstance(BoA, str) else BoA
    call = lambda: F.fdtd(cs["c"], cs["rho"], cs["z"], cs["x"], positions(cs, "src"), cs["nrm"], kw.pop("s", cs["s"]), positions(cs, "sen"), kw.pop("Nt", cs["Nt"]),
                          cs["dt"], PML=cs["P"], order=2 * R_, prec=prec, return_state=True, loss=block(ls), BoA=BoA, **kw)
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
        print(f"fdtd nl ratio {what} {name}: err {err:.3e}, d32 {d32[name]:.3e}, tol {tol:.3e}, ratio {err / tol:.3f}")
        if not err <= tol:
            bad.append((name, err, tol))
    SEEN["ratio"] = max(SEEN["ratio"], worst)
    print(f"fdtd nl ratio {what}: {worst:.3f} (largest so far {SEEN['ratio']:.3f})")
    assert not bad, (what, bad)


# ---------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("grid,R_,V,L,prec", CASES, ids=lambda v: "x".join(str(k) for k in v) if isinstance(v, tuple) else str(v))
def test_parity_with_the_restatement(grid, R_, V, L, prec, monkeypatch):
    cs, ls, r64, _, d32 = NR.parity_refs(*grid, R_, V, L)
    rec, st = run_case(cs, ls, R_, prec, monkeypatch)
    assert rec.dtype == (torch.float32 if prec == "single" else torch.float64) and tuple(rec.shape) == (cs["Nt"], len(cs["sen"][0]), V)
    assert ("e" in st) == bool(L) and (not L or tuple(st["e"].shape) == (V, L) + tuple(st["p"].shape[1:]))
    compare(rec, st, r64, d32, prec == "double", f"{grid} R = {R_} V = {V} L = {L} {prec}")


@pytest.mark.parametrize("L", NR.LOSSES, ids=lambda L: f"L{L}")
def test_parity_without_the_convective_term(L):
    grid = (37, 29, 6)
    cs, ls, r64, _, d32 = NR.parity_refs(*grid, 4, 3, L, K=0.0)
    rec, st = run_case(cs, ls, 4, "single", convective=False)
    compare(rec, st, r64, d32, False, f"{grid} K = 0 L = {L}")
    on, _ = run_case(cs, ls, 4, "single")
    assert not ST.same_bits(on, rec)


# ---------------------------------------------------------------------------------------------------------------- the bit pins
@pytest.mark.parametrize("R_,prec", [(4, "single"), (4, "double"), (1, "single"), (2, "double"), (2, "single"), (1, "double")])
@pytest.mark.parametrize("L", [None, 0, 1, 2, 3, 4], ids=lambda L: f"L{L}")
def test_a_zero_block_gives_the_bits_of_the_linear_entries(L, R_, prec):
    """QDAS_FDTD_NL_NO_CONVECTIVE and an all-zero bq: the bits of qdas_fdtd without a loss block and of qdas_fdtd_lossy with one -- the nonlinear pass states
    the roundings of both (csrc/fdtd_core.h), for every order, both precisions and every count of mechanisms"""
    cs = NR.nl_case(37, 29, 6, 3)
    ls = None if L is None else LR.loss_case(37, 29, L, cs["dt"])
    want, ws = run_case(cs, ls, R_, prec, BoA=None)
    got, gs = run_case(cs, ls, R_, prec, BoA=np.zeros_like(cs["BoA"]), convective=False)
    for k in ws:
        assert ST.same_bits(gs[k], ws[k]), k
    assert ST.same_bits(got, want) and set(gs) == set(ws)
    # and each term on its own leaves them
    conv, _ = run_case(cs, ls, R_, prec, BoA=0.0)
    quad, _ = run_case(cs, ls, R_, prec, convective=False)
    assert not ST.same_bits(conv, want) and not ST.same_bits(quad, want) and not ST.same_bits(conv, quad)


def test_BoA_none_and_all_nan_dispatch_the_old_entries(monkeypatch):
    cs = NR.nl_case(37, 29, 6, 3)
    seen = []
    real = _lib.lib

    class Spy:
        def __getattr__(self, name):
            if name.startswith("qdas_fdtd") and "tile" not in name:
                seen.append(name)
            return getattr(real(), name)

    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    for BoA, ls, want in ((None, None, "qdas_fdtd"), (np.full((37, 29), np.nan), None, "qdas_fdtd"), (float("nan"), LR.loss_case(37, 29, 3, cs["dt"]), "qdas_fdtd_lossy"),
                          (0.0, None, "qdas_fdtd_nonlinear"), (cs["BoA"], LR.loss_case(37, 29, 0, cs["dt"]), "qdas_fdtd_nonlinear")):
        seen.clear()
        run_case(cs, ls, 4, "single", BoA=BoA)
        assert seen == [want], (want, seen)


@pytest.mark.parametrize("L", [None, 3], ids=lambda L: f"L{L}")
def test_two_runs_give_the_same_bits(L):
    cs = NR.nl_case(37, 29, 6, 3)
    ls = None if L is None else LR.loss_case(37, 29, L, cs["dt"])
    a, sa = run_case(cs, ls, 4, "single")
    b, sb = run_case(cs, ls, 4, "single")
    assert ST.same_bits(a, b) and all(ST.same_bits(sa[k], sb[k]) for k in sa)


def _prepared(cs, ls, order=8, **kw):
    return F.fdtd(cs["c"], cs["rho"], cs["z"], cs["x"], positions(cs, "src"), cs["nrm"], cs["s"], positions(cs, "sen"), cs["Nt"], cs["dt"], PML=cs["P"],
                  order=order, prepare_only=True, loss=block(ls), BoA=cs["BoA"], **kw)


def _fresh(meta, V, L, fill=0.0):
    st = {k: torch.full((V, meta["Nx"], meta["ld"]), fill, dtype=torch.float32, device="cuda") for k in F.STATES}
    st["e"] = torch.full((V, L, meta["Nx"], meta["ld"]), fill, dtype=torch.float32, device="cuda")
    return st, torch.empty((meta["Nt"], meta["N"], V), dtype=torch.float32, device="cuda")


def test_the_tables_and_the_meta_of_prepare_only():
    cs = NR.nl_case(37, 29, 6, 3)
    meta, tb, _ = _prepared(cs, LR.loss_case(37, 29, 3, cs["dt"]))
    assert meta["nl"] == dict(convective=True, beta_max=1.0 + NR.BOA_MAX / 2.0) and meta["loss"]["L"] == 3 and "kap" in tb
    want = np.pad(cs["bq"], 6, mode="edge").T.astype(np.float32)
    assert tuple(tb["bq"].shape) == (41, 49) and tb["bq"].dtype == torch.float32 and np.array_equal(tb["bq"].cpu().numpy(), want)
    meta, tb, _ = F.fdtd(cs["c"], cs["rho"], cs["z"], cs["x"], positions(cs, "src"), cs["nrm"], cs["s"], positions(cs, "sen"), cs["Nt"], cs["dt"], PML=6,
                         prepare_only=True, BoA=2.0, convective=False, prec="double")
    assert meta["nl"] == dict(convective=False, beta_max=1.0) and "loss" not in meta and "kap" not in tb and tb["bq"].dtype == torch.float64
    meta, tb, _ = F.fdtd(cs["c"], cs["rho"], cs["z"], cs["x"], positions(cs, "src"), cs["nrm"], cs["s"], positions(cs, "sen"), cs["Nt"], cs["dt"], PML=6,
                         prepare_only=True, BoA=np.full((37, 29), np.nan))
    assert "nl" not in meta and "bq" not in tb


def test_a_nan_in_one_pulse_stays_there():
    cs = NR.nl_case(37, 29, 6, 3)
    ls = LR.loss_case(37, 29, 3, cs["dt"])
    meta, tb, s_dev = _prepared(cs, ls)
    out = []
    for poison in (False, True):
        st, rec = _fresh(meta, 3, 3)
        if poison:
            st["rz"][1, 20, 24] = float("nan")                    # one node of the middle pulse: ro carries it into the convective term
        F.launch(meta, tb, st, s_dev, rec, 0)
        torch.cuda.synchronize()
        out.append((rec, st))
    (clean, sc), (bad, sb) = out
    for v in (0, 2):
        assert ST.same_bits(clean[:, :, v], bad[:, :, v]) and all(ST.same_bits(sc[k][v], sb[k][v]) for k in sc)
    assert torch.isnan(bad[:, :, 1]).any() and torch.isnan(sb["p"][1]).any() and torch.isnan(sb["e"][1]).any()
    # and a NaN in one pulse's column of the source table
    s_bad = s_dev.clone()
    s_bad[3, :, 2] = float("nan")
    st, rec = _fresh(meta, 3, 3)
    F.launch(meta, tb, st, s_bad, rec, 0)
    torch.cuda.synchronize()
    assert ST.same_bits(rec[:, :, :2], clean[:, :, :2]) and torch.isnan(rec[:, :, 2]).any()


def test_the_entry_clears_the_states_and_the_memory_variables_when_asked():
    """QDAS_FDTD_ZERO: NaN-filled states and ``e`` with a padded row stride give the bits of a start from zeroed ones, and the padding keeps its poison"""
    cs = NR.nl_case(49, 33, 8, 2)
    for L in (None, 2):
        ls = None if L is None else LR.loss_case(49, 33, L, cs["dt"])
        meta, tb, s_dev = _prepared(cs, ls, ld=70)
        out = []
        for fill, flags in ((0.0, 0), (float("nan"), _lib.FDTD_ZERO)):
            st, rec = _fresh(meta, 2, L or 0, fill)
            if L is None:
                del st["e"]
            F.launch(dict(meta, flags=flags), tb, st, s_dev, rec, 0)
            torch.cuda.synchronize()
            out.append((rec, st))
        assert ST.same_bits(out[0][0], out[1][0]) and all(ST.same_bits(out[0][1][k][..., :65], out[1][1][k][..., :65]) for k in out[0][1])
        assert all(bool(torch.isnan(out[1][1][k][..., 65:]).all()) for k in out[1][1])
        assert float(out[0][0].abs().max()) > 0


@pytest.mark.parametrize("prec,L", [("single", 3), ("double", None), ("single", 0)])
def test_strided_states_with_guard_bands(prec, L, monkeypatch):
    """``ld = Nz + 7``: the record, the states and ``e`` sit between guard bands (``run_case`` checks them), and the row padding is never written"""
    grid = (37, 29, 6)
    cs, ls, r64, _, d32 = NR.parity_refs(*grid, 4, 3, L)
    rec, st = run_case(cs, ls, 4, prec, monkeypatch, ld=49 + 7)
    assert st["p"].stride(1) == 56 and (not L or st["e"].stride() == (L * 41 * 56, 41 * 56, 56, 1))
    compare(rec, st, r64, d32, prec == "double", f"{grid} ld = Nz + 7 L = {L} {prec}")


def test_blocks_of_pulses_give_the_same_bits(monkeypatch):
    cs = NR.nl_case(37, 29, 6, 3)
    ls = LR.loss_case(37, 29, 3, cs["dt"])
    a, sa = run_case(cs, ls, 4, "single", bsize=3)
    b, sb = run_case(cs, ls, 4, "single", bsize=1)
    c_, sc = run_case(cs, ls, 4, "single", bsize=2)
    assert ST.same_bits(a, b) and ST.same_bits(a, c_) and all(ST.same_bits(sa[k], sb[k]) and ST.same_bits(sa[k], sc[k]) for k in NAMES)
    # without return_state ONE set of 5 + L arrays of bsize pulses serves every block: the record, five states and e
    with GD.guard_outputs(monkeypatch) as g:
        rec = F.fdtd(cs["c"], cs["rho"], cs["z"], cs["x"], positions(cs, "src"), cs["nrm"], cs["s"], positions(cs, "sen"), cs["Nt"], cs["dt"], PML=6, order=8,
                     loss=block(ls), BoA=cs["BoA"], bsize=2)
        assert g.check(rec) == 1
    shapes = sorted(tuple(b_.inner.shape) for b_ in g.bufs)
    assert shapes == sorted([(cs["Nt"], 4, 3)] + [(2, 41, 49)] * 5 + [(2, 3, 41, 49)]), shapes
    assert ST.same_bits(rec, a)


def test_stream_delayed_producer_on_a_side_stream():
    from tests.test_gpu_raybackproject import own_stream
    grid, L = (37, 29, 6), 3
    cs, ls, r64, _, d32 = NR.parity_refs(*grid, 4, 3, L)
    meta, tb, s_dev = _prepared(cs, ls)
    names = list(tb)
    assert "bq" in names and "kap" in names
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
    q = _lib.FdtdNl()
    assert L.qdas_fdtd_nonlinear(C.byref(d), None, None, C.byref(q)) == 0           # null pointers: a launch would have been refused or would fault
    d.Nt, d.V = 10, 0
    assert L.qdas_fdtd_nonlinear(C.byref(d), None, None, C.byref(q)) == 0
    cs = NR.nl_case(37, 29, 6, 3)
    ls = LR.loss_case(37, 29, 2, cs["dt"])
    rec, st = run_case(cs, ls, 4, "single", Nt=0)
    assert tuple(rec.shape) == (0, 4, 3) and all(float(st[k].abs().max()) == 0.0 for k in NAMES)
    rec, st = run_case(cs, None, 4, "single", s=np.zeros((R.TS, len(cs["src"][0]), 0)))
    assert tuple(rec.shape) == (cs["Nt"], 4, 0) and "e" not in st and tuple(st["p"].shape) == (0, 41, 49)


# ---------------------------------------------------------------------------------------------------------------- quadratic scaling
def test_pulse_inversion_sums_vanish_without_BoA_and_scale_quadratically_with_it():
    cs = NR.nl_case(37, 29, 6, 1)
    s4 = cs["s"] * np.array([0.5, -0.5, 1.0, -1.0])[None, None, :]
    lin, _ = run_case(cs, None, 4, "single", BoA=None, s=s4)
    assert float(lin.abs().max()) > 0
    assert not (lin[:, :, 0] + lin[:, :, 1]).any() and not (lin[:, :, 2] + lin[:, :, 3]).any(), "the linear solver is odd in its sources, bit for bit"
    rec, _ = run_case(cs, None, 4, "single", s=s4)
    rec = rec.double().cpu().numpy()
    s1, s2 = rec[:, :, 0] + rec[:, :, 1], rec[:, :, 2] + rec[:, :, 3]
    dev = np.abs(s2 - 4 * s1).max() / np.abs(4 * s1).max()
    print(f"fdtd nl quadratic scaling: max|S(A)| / max|rec| {np.abs(s1).max() / np.abs(rec).max():.3e}, |S(2A) - 4 S(A)| / |4 S(A)| {dev:.3e}, bound {2 * QUAD_DEV:.3e}")
    assert np.abs(s1).max() > 1e-4 * np.abs(rec).max() and dev <= 2 * QUAD_DEV


# ---------------------------------------------------------------------------------------------------------------- physics
_PHYS = {}


def _physics_record(K):
    """the Fubini case on the device in float32: ``prepare_only``, ``dt / rho_sgx`` set to 0 (every column a 1-D line), one launch"""
    if K not in _PHYS:
        ps = NR.physics_setup()
        z, x = np.arange(ps["Z"]) * ps["h"], (np.arange(ps["X"]) - ps["X"] // 2) * ps["h"]
        pos = lambda pts: np.stack([z[pts[0]], x[pts[1]]])
        meta, tb, s_dev = F.fdtd(ps["c"], ps["rho"], z, x, pos(ps["src"]), ps["nrm"], ps["s"], pos(ps["sen"]), ps["Nt"], ps["dt"], PML=ps["P"], order=2 * ps["R"],
                                 prepare_only=True, BoA=ps["BoA"], convective=K != 0.0)
        tb["dtrx"].zero_()
        st = {k: torch.zeros((1, meta["Nx"], meta["ld"]), dtype=torch.float32, device="cuda") for k in F.STATES}
        rec = torch.empty((meta["Nt"], meta["N"], 1), dtype=torch.float32, device="cuda")
        F.launch(meta, tb, st, s_dev, rec, 0)
        torch.cuda.synchronize()
        assert not st["ux"].any() and not st["rx"].any()
        _PHYS[K] = (ps, rec[:, :, 0].double().cpu().numpy())
    return _PHYS[K]


@pytest.mark.parametrize("name", list(VARIANTS))
def test_the_device_follows_fubini(name):
    assert set(PHYS_DEV) == set(VARIANTS)
    ps, rec = _physics_record(VARIANTS[name][0])
    assert np.abs(rec[:, 0]).max() == pytest.approx(NR.P0, rel=0.03)
    check_fubini(name, rec, ps, "device, float32")


# ---------------------------------------------------------------------------------------------------------------- end to end
E2E_LEVEL_DB = -17.36              # the float64 restatement on the CPU (the docstring below)


def test_tissue_harmonic_image_through_das():
    """fdtdSim(BoA = 6, alpha = 0.5) twice, with the waveform and with its inverse -> half difference (fundamental) and half sum (second harmonic) -> hilbert ->
    DAS.  The harmonic image peaks within one pixel of the fundamental image's peak, and its level relative to the fundamental image is within 1 dB of the
    float64 restatement's (``E2E_LEVEL_DB``; the 1 dB is for float32 and cubic against linear interpolation in DAS; parity carries the precision).

    The float64 restatement on the CPU (tests/fdtd_nl_ref.py ``simulate`` with the plan's tables, both pulses and both media, a numpy DAS with linear
    interpolation at 140 MHz) gave, on the image's pixels of 0.15 mm (a quarter wavelength): fundamental peak 3.64e5 at z = 11.95 mm, x = 0; harmonic peak
    4.94e4 at z = 11.80 mm, x = 0: -17.36 dB.  On a line of 0.01 mm steps through x = 0 the envelopes peak at 11.90 and 11.82 mm: the harmonic's sits 0.08 mm
    shallower, half a pixel, which is why the pixel is not finer.  The largest ``|u| / c`` was 7.8e-3 (beside the source nodes), the largest pressure 3.9 MPa
    there; the plan's source Mach number is 1.6e-3."""
    us, c, rho, cgrd, kw, zi, xi = NR.e2e_setup()
    plus = us.fdtdSim(c, rho, cgrd, **kw)
    minus = us.fdtdSim(c, rho, cgrd, **dict(kw, waveform=-kw["waveform"]))
    assert plus.fs == minus.fs == 140e6 and plus.t0 == minus.t0
    image = lambda y: us.DAS(ChannelData(y, plus.t0, plus.fs, "TNM").hilbert(), c0=NR.E2E["C0"]).abs().reshape(len(zi), len(xi)).double().cpu().numpy()
    kf, kh, level = NR.harmonic_level(image(0.5 * (plus.data - minus.data)), image(0.5 * (plus.data + minus.data)))
    print(f"fdtd nl end to end: fundamental peak at pixel {tuple(int(v) for v in kf)} (z {zi[kf[0]] * 1e3:.2f} mm, x {xi[kf[1]] * 1e3:.2f} mm), harmonic peak at "
          f"{tuple(int(v) for v in kh)} (z {zi[kh[0]] * 1e3:.2f} mm, x {xi[kh[1]] * 1e3:.2f} mm), harmonic level {level:.2f} dB (restatement {E2E_LEVEL_DB:.2f} dB)")
    assert abs(kf[0] - kh[0]) <= 1 and abs(kf[1] - kh[1]) <= 1
    assert abs(level - E2E_LEVEL_DB) <= 1.0
