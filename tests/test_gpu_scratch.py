"""Memory the library owns itself: the per-stream arenas of csrc/scratch.hip, the scratch of a plan, and the pointer-keyed memo of qdas_das_lut.

No torch tensor reaches that memory, so neither the guard bands of tests/test_gpu_guards.py nor the delayed producer of tests/test_gpu_streams.py sees it, and
it is where state survives from one call to the next.  The audit behind this file -- every region handed out by ``Scratch::get`` and every plan-owned buffer
that is not wholly uploaded, with its first writer and its readers -- is the table of DESIGN.md section 5d.  The cases are the rows of
``tests/test_gpu_streams.py`` ``CASES`` (builders are not copied); ``ARENA_USERS`` below maps every source file that constructs a ``Scratch`` to the rows
that reach it, and tests/test_scratch_host.py holds that map against csrc/*.hip.

1. POISON.  ``QDAS_SCRATCH_POISON=255`` (read per call) fills every block of ``Scratch::get`` on the call's stream and every plan-owned allocation at
   allocation.  Per row: ``qdas_device_trim``, a clean run, then the builder entered again under the switch (plans are created under it) and a second run.
   ``exact`` rows must agree bit for bit; rows that accumulate with float atomics must meet their home file's bound against their own oracle, as in
   tests/test_gpu_streams.py.  The five ``arena0-*`` rows do the same down the per-call-block path.  No tolerance of this file's own.
2. WAKE.  The seven arena users on one stream, in a fixed order and in the reverse one, without poison: each result against the same call issued alone
   after a trim.  This is the pipeline condition (another entry's tables in the arena) and regrows the arena between unlike sizes.
3. HISTORY.  Every plan row: frame A, the all-NaN frame (bytes 0xFF), frame A again on one plan; the third image equals the first and holds no NaN.  The
   rows that stream frames also vary the frame count on one plan (4, 1, 3, 2) against fresh plans.
4. MEMO.  qdas_das_lut through the C ABI on two table tensors that are refreshed IN PLACE: memo hit, symmetry broken by one ulp, restored, a slope that
   misfits the remembered footprint, back, and a slope no mirror footprint fits.  The slopes come from the fit rule of csrc/tile_prologue.h (below).

Layouts a row is here for (all at the home files' sizes unless a threshold asks for more):
das_lut partial images (``ks > 1``: 3 tiles < CUs) -- das_lut-sum-single; the mirror build with ``ks2 = 8`` -- das_lut-mirror; greens' arena is reached by the
impulse-train kernels only (>= 2048 entries or QDAS_GREENS_TRAIN_MIN=0: greens-single / -double never touch it) -- greens-trains (no sort), greens-trains-sorted
(>= 4096 scatterers); adjoint partial images with ``kchunks > 1`` -- adjoint-sum (few pixel tiles), per-pixel ``w1`` -- adjoint-keep_tx (norms), -keep_rx
(normalised fields); migration with several slices -- migration-* (K < 512 columns), ``keep_tx`` -- migration-blocks-keep_tx; eikonal with reused chunk
counters -- eikonal-chunks (asserts more than four passes); shift_sum in fp64 with and without weights -- shift_sum-double, -double-noweights; a plan with
misfit tiles -- das-misfit; a lateral-mirror plan -- das-mirror.

What this cannot see: a read of stale bytes whose value is discarded by a select; arenas of other devices (one GPU here)."""
import contextlib
import ctypes as C
import re

import numpy as np
import pytest
import torch

from tests import streams as ST
from tests import test_gpu_streams as S
from tests.cases import rel_err
from tests.streams import same_bits

pytestmark = pytest.mark.gpu

POISON = "255"

# csrc file that constructs a Scratch -> the rows of tests/test_gpu_streams.py CASES that reach its regions (DESIGN.md 5d has one table row per region)
ARENA_USERS = {
    "das_lut.hip": ["das_lut-sum-single", "das_lut-rx", "das_lut-tx", "das_lut-mirror"],
    "shiftsum.hip": ["shift_sum-host-tables", "shift_sum-device-tables", "shift_sum-double", "shift_sum-double-noweights"],
    "greens.hip": ["greens-trains", "greens-trains-sorted"],
    "pre.hip": ["convd-fft"],                                          # (fftconv_launch: qdas_convd's FFT path)
    "migration.hip": ["migration-0", "migration-1", "migration-blocks", "migration-blocks-keep_tx", "migration-compose"],
    "adjoint.hip": ["adjoint-sum", "adjoint-sum-blocks", "adjoint-keep_tx", "adjoint-keep_rx"],
    "eikonal.hip": ["eikonal", "eikonal-chunks"],
}
ARENA_ROWS = [cid for ids in ARENA_USERS.values() for cid in ids]
ARENA0_ROWS = [cid for cid, (e, _, _, _) in S.CASES.items() if e == "arena0"]
PLAN_ROWS = [cid for cid, (e, _, _, _) in S.CASES.items() if e in ("das_plan", "sharded", "oneshot_das")]
WAKE = ["das_lut-sum-single", "shift_sum-device-tables", "greens-trains", "convd-fft", "migration-1", "adjoint-sum", "eikonal"]      # one row per arena user


def _trim():
    from qups_amd import _lib
    torch.cuda.synchronize()
    assert _lib.lib().qdas_device_trim() == 0


def _keep(r):
    torch.cuda.synchronize()
    return tuple(o.clone() for o in ST._tup(r))


def _agree(cid, got, want, verify, what):
    assert len(got) == len(want), (cid, what)
    if S.CASES[cid][1]:
        bad = [k for k, (a, b) in enumerate(zip(got, want)) if not same_bits(a, b)]
        assert not bad, f"{cid}: {what}"
    else:                                                             # (float atomics: the home file's own bound against its own oracle)
        verify(got[0] if len(got) == 1 else got)


def _has_nan(o):
    return bool(torch.isnan(torch.view_as_real(o) if o.is_complex() else o).any())


def _no_nan(cid, outs, what):
    for o in outs:
        assert not _has_nan(o), f"{cid}: NaN in the result ({what})"


# ================================================================================================================ 1. poison
@pytest.mark.parametrize("cid", ARENA_ROWS + PLAN_ROWS + ARENA0_ROWS)
def test_poisoned_scratch_changes_nothing(cid, monkeypatch):
    monkeypatch.delenv("QDAS_SCRATCH_POISON", raising=False)
    builder = S.CASES[cid][3]
    _trim()
    with builder() as c:
        clean = _keep(c["fn"](*c["tensors"]))
    monkeypatch.setenv("QDAS_SCRATCH_POISON", POISON)                  # before the builder is entered: its plans are created under the switch
    with builder() as c:
        got = _keep(c["fn"](*c["tensors"]))
        again = _keep(c["fn"](*c["tensors"]))                         # (the arena now has its size: the block of the first call, poisoned anew)
        if "route" in c:
            assert c["fn"].kernel.startswith(c["route"]), (cid, c["fn"].kernel)
        for r in (got, again):
            _agree(cid, r, clean, c.get("verify"), "the result changes when the library's scratch is filled with 0xFF before use: something reads a temporary that "
                                                   "its own call has not written")
            _no_nan(cid, r, "poisoned scratch")


def test_the_greens_rows_run_the_train_kernels():
    """only the impulse-train kernels of csrc/greens.hip take scratch: QDAS_GREENS_TRAIN_MIN=0 must select them (the per-sample kernel gives other bits)"""
    with S.CASES["greens-trains"][3]() as c:
        a, b = _keep(c["fn"]("0")), _keep(c["fn"]("1000000000000"))
    assert not same_bits(a[0], b[0]), "QDAS_GREENS_TRAIN_MIN=0 did not select the impulse-train kernels: the greens rows do not reach the arena"


def test_the_switch_fills_every_kind_of_block(monkeypatch):
    """the harness can fail: with QDAS_SCRATCH_POISON set, the first and the last byte of a block from each path of ``Scratch::get`` -- per-call blocks of a call
    that outgrows the (trimmed) arena, the regrown arena, never-kept blocks (QDAS_SCRATCH_ARENA_MAX_MB=0) -- hold that byte; other values are refused"""
    from qups_amd import _lib
    L = _lib.lib()
    f = L.qdas_debug_scratch_peek
    f.argtypes, f.restype = [C.c_size_t, C.c_void_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)], C.c_int
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def peek(n):
        a, b = C.c_ubyte(0), C.c_ubyte(0)
        assert f(n, st, C.byref(a), C.byref(b)) == 0
        return a.value, b.value
    for val in ("165", "0x5a"):
        monkeypatch.setenv("QDAS_SCRATCH_POISON", val)
        want = int(val, 0)
        _trim()
        assert peek(1000) == (want, want), "per-call block of a call that outgrew the arena"
        assert peek(1000) == (want, want) and peek(257) == (want, want), "the arena"
        monkeypatch.setenv("QDAS_SCRATCH_ARENA_MAX_MB", "0")
        assert peek(1000) == (want, want), "never-kept block"
        monkeypatch.delenv("QDAS_SCRATCH_ARENA_MAX_MB")
    monkeypatch.setenv("QDAS_SCRATCH_POISON", "165")
    peek(1000)
    for val in ("", "256", "-1", "ff", "12x"):                        # not a byte value: the switch is off, the block keeps what it held (165 from the line above)
        monkeypatch.setenv("QDAS_SCRATCH_POISON", val)
        assert peek(1000) == (165, 165), val
    monkeypatch.setenv("QDAS_SCRATCH_POISON", "7")
    assert peek(1000) == (7, 7)


# ================================================================================================================ 2. wake
def test_arena_users_in_each_others_wake():
    with contextlib.ExitStack() as es:
        cs = [es.enter_context(S.CASES[cid][3]()) for cid in WAKE]
        solo = []
        for c in cs:
            _trim()
            solo.append(_keep(c["fn"](*c["tensors"])))
        for order in (range(len(WAKE)), reversed(range(len(WAKE)))):
            _trim()                                                   # the arena starts empty and regrows from one entry's size to the next's
            outs = {}
            for k in order:
                outs[k] = ST._tup(cs[k]["fn"](*cs[k]["tensors"]))     # (no synchronisation of this test's own between the calls)
            torch.cuda.synchronize()
            for k, r in outs.items():
                _agree(WAKE[k], r, solo[k], cs[k].get("verify"), "the result differs from the same call issued alone: it read what another entry left in the arena")


# ================================================================================================================ 3. history
@pytest.mark.parametrize("cid", PLAN_ROWS)
def test_plans_keep_no_history(cid):
    with S.CASES[cid][3]() as c:
        fn, t, verify = c["fn"], list(c["tensors"]), c.get("verify")
        nan = [ST._poisoned_twin(t[0])] + t[1:]                         # the data is the first tensor of every plan row; geometry stays
        rA = _keep(fn(*t))
        rN = _keep(fn(*nan))
        r3 = _keep(fn(*t))
        assert any(_has_nan(o) for o in rN), f"{cid}: the NaN frame left no NaN: the test does not see the data path"
        _agree(cid, r3, rA, verify, "frame A after a NaN frame differs from frame A on the fresh plan: the plan carried something over")
        _no_nan(cid, r3, "frame A after a NaN frame")
        if "frames" not in c:
            return
        # the frame count varies on ONE plan; every count against a fresh plan of the same problem
        x = t[0] if c["frames"] == 4 else torch.cat([t[0], t[0] * (0.5 - 0.25j)])
        assert x.shape[0] == 4
        for k in (4, 1, 3, 2):
            xk = x[:k].contiguous()
            got = _keep(c["plan"].execute_colmajor(xk, k))
            with c["fresh"]() as p:
                want = _keep(p.execute_colmajor(xk, k))
            assert same_bits(got[0], want[0]), f"{cid}: {k} frames on a plan that has streamed other counts differ from {k} frames on a fresh plan"
            _no_nan(cid, got, f"{k} frames")


# ================================================================================================================ 4. the memo of qdas_das_lut
# The fit rule (csrc/tile_prologue.h): a tile fits when a_ext + b_ext + K + 1 <= W, with W = probe_w = 128 for the mirror build, K = 4 taps (cubic), and per
# table ext = (mx + dlt) - (floor(mn - dlt) - 1) + 0.01 for the element whose delays spread most over the tile's pixels, dlt = 1e-6 (max|delay| + 2) <= 1.1e-3
# here.  With spread = mx - mn: spread + 1.01 <= ext < spread + 2.013, so with S = the two tables' spreads added
#     S <= 118.97  ->  the tile fits for certain;      S > 120.98  ->  it misfits for certain.
# A footprint of level l is 2^l rows x (1024 >> l) columns (16 waves); the mirror build tiles the first 20 of the 40 columns: 64 x 16, 32 x 20, 16 x 20, 8 x 20.
# tests/test_gpu_streams.py lut_mirror_tables: spread of one table = a (rows - 1) + lat (columns - 1).  With A = a_rx + a_tx:
#     gentle  A = 1, lat = 0.05:  l = 6: 63 + 1.5 = 64.5                         fits the first footprint tried (64 rows)
#     steep   A = 3, lat = 0.05:  l = 6: 189 + 1.5 = 190.5 misfits;  l = 5: 93 + 1.9 = 94.9 fits
#     wide    A = 6, lat = 2.5:   l = 6: 378 + 75;  l = 5: 186 + 95;  l = 4: 90 + 95;  l = 3: 42 + 95 = 137: every footprint misfits
# Largest delay (wide): 2 (4 + 3 x 139 + 2.5 x 19 + 0.03 x 31) = 938.9 < T - 3: every pixel samples inside the record in all three.
GENTLE, STEEP, WIDE = (0.5, 0.5, 0.05), (1.5, 1.5, 0.05), (3.0, 3.0, 2.5)
LUT_TOL = 2e-5                                                         # tests/test_gpu_golden.py test_das_lut_mirror_symmetric_tables_take_the_mirror_mode


def test_das_lut_tables_refreshed_in_place(monkeypatch):
    from oracle import das_oracle as O
    from qups_amd import _lib
    from qups_amd.das_spec import _PREC
    for v in ("QDAS_LUT_NO_MIRROR", "QDAS_NO_MIRROR", "QDAS_NO_JIT", "QDAS_LUT_GENERIC", "QDAS_SCRATCH_POISON"):
        monkeypatch.delenv(v, raising=False)
    L = _lib.lib()
    T, N, M, I1, I2 = 1024, 32, 32, 140, 40
    I = I1 * I2
    xh = S.lut_mirror_data(T, N, M)
    x = torch.from_numpy(np.ascontiguousarray(xh.transpose(2, 1, 0))).cuda()                      # (M, N, T): column-major T x N x M
    lay = lambda a: torch.from_numpy(np.ascontiguousarray(a.transpose(2, 1, 0)))                   # I1 x I2 x E -> (E, I2, I1)
    tabs = {k: S.lut_mirror_tables(*v) for k, v in (("gentle", GENTLE), ("steep", STEEP), ("wide", WIDE))}
    rx, tx = lay(tabs["gentle"][0]).cuda(), lay(tabs["gentle"][1]).cuda()                         # THE two table tensors: the same pointers throughout
    y = torch.empty(I, dtype=torch.complex64, device="cuda")
    d = _lib.LutDesc()
    d.T, d.N, d.M, d.I, d.I1 = T, N, M, I, I1
    d.flag, d.dtype, d.omega = _lib.INTERP_FLAGS["cubic"], _PREC["single"], 0.0
    d.tau_rx, d.tau_tx = rx.data_ptr(), tx.data_ptr()
    buf = C.create_string_buffer(200)
    L.qdas_das_lut_last_kernel.argtypes = [C.c_char_p, C.c_size_t]

    def call():
        torch.view_as_real(y).fill_(float("nan"))
        torch.cuda.synchronize()
        _lib.check(L.qdas_das_lut(C.byref(d), C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        assert L.qdas_das_lut_last_kernel(buf, 200) == 0
        assert not bool(torch.isnan(torch.view_as_real(y)).any()), "a pixel was not rewritten by this call (" + buf.value.decode() + ")"
        return y.clone(), buf.value.decode()

    def put(name):
        rx.copy_(lay(tabs[name][0]))
        tx.copy_(lay(tabs[name][1]))

    def oracle(trx, ttx):
        return np.asarray(O.das_lut(xh, trx.astype(np.float64), ttx.astype(np.float64), 0.0, 1.0, interp="cubic")).reshape(I1, I2).reshape(-1, order="F")

    def err(yy, ref):
        e = rel_err(yy.cpu().numpy(), ref)
        print(f"das_lut in place: rel_err={e:.3e}")
        return e
    key = lambda name: re.search(r"\[jit ([^\]]+)\]", name).group(1)
    ref_gentle = oracle(*tabs["gentle"])

    y1, k1 = call()                                                   # 1. symmetric, gentle
    if "mirror" not in k1:                                            # (no hiprtc on this box: the mode exists as a specialised build only)
        pytest.skip("no mirror build: " + k1)
    assert k1.startswith("tiled,mirror") and "[jit " in k1, k1
    assert err(y1, ref_gentle) <= LUT_TOL
    y2, k2 = call()                                                   # 2. the memo hit
    assert k2 == k1 and same_bits(y2, y1)
    moved = tabs["gentle"][0].copy()                                  # 3. one receive entry one ulp off, in place
    moved[17, 3, 5] = np.nextafter(moved[17, 3, 5], np.float32(np.inf))
    rx[5, 3, 17:18].copy_(torch.from_numpy(moved[17, 3, 5:6].copy()))
    y3, k3 = call()
    assert k3 == "tiled", k3
    monkeypatch.setenv("QDAS_LUT_NO_MIRROR", "1")
    y3b, k3b = call()
    monkeypatch.delenv("QDAS_LUT_NO_MIRROR")
    assert k3b == "tiled" and same_bits(y3, y3b), "the redo after a stale mirror launch differs from the general kernel's own image"
    assert err(y3, oracle(moved, tabs["gentle"][1])) <= LUT_TOL
    put("gentle")                                                     # 4. symmetry restored
    y4, k4 = call()
    assert k4 == k1 and same_bits(y4, y1), k4
    put("steep")                                                      # 5. the remembered 64-row footprint misfits, 32 rows fit
    y5, k5 = call()
    assert k5.startswith("tiled,mirror") and key(k5) != key(k1), (k1, k5)
    assert err(y5, oracle(*tabs["steep"])) <= LUT_TOL
    put("gentle")                                                     # 6. back: the remembered shallower footprint verifies (another summation split than step 1)
    y6, k6 = call()
    assert k6.startswith("tiled,mirror"), k6
    assert err(y6, ref_gentle) <= LUT_TOL
    put("wide")                                                       # 7. no mirror footprint fits
    y7, k7 = call()
    assert "mirror" not in k7, k7
    assert err(y7, oracle(*tabs["wide"])) <= LUT_TOL
