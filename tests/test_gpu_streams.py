"""Every device entry on a NON-BLOCKING side stream with work queued in front of it (helpers: tests/streams.py).

include/qdas.h promises, per entry that takes ``void *stream``: "asynchronous on ``stream``" / "one launch on ``stream``, no synchronisation" / "WAITS for the
stream", and "keep x / y alive until the stream has passed the call".  The rest of the GPU suite runs on torch's default stream, which every blocking stream
synchronises with: an internal step on the wrong stream is invisible there.  Here each row of ``CASES`` is run

1. twice on the default stream (``exact`` rows: the two runs must agree bit for bit),
2. twice on the side stream (warm: the stream's arena of csrc/scratch.hip exists and has its size, memo tables and plans exist),
3. behind the DELAYED PRODUCER: every device input is an all-0xFF twin that receives the true data on the side stream behind ``FILL_MS`` of fills; directly
   behind the call, still without a synchronisation, every output is cloned on the side stream (the consumer).  Output and clone must both be
   bit-identical to the serial result (``exact=True``) or meet the home test file's own parity bound against its own oracle (``exact=False``: entries that
   accumulate with float atomics), imported from there.  No new tolerance appears in this file.
4. EARLY RETURN: the wrapper must have returned while the filler was still running, unless its entry is listed in ``BLOCKS`` with the place that waits; an entry
   in ``BLOCKS`` that returns early fails too (the table must stay true).

Rows marked ``inter`` also go through ``streams.interleaved`` (probabilistic for a shared temporary; see tests/streams.py).

FILL_MS: the largest host wall time of a warm wrapper call on the default stream, measured on the MI355X inside this module (``QDAS_STREAMS_MEASURE=1`` reports
every case's and asserts no early return; every run prints them), was 1.56 ms (migration-compose; 1.46 and 0.91 ms, bfAdjoint, in two later runs); FILL_MS is ten
times that, rounded up: 16.  The interleaved groups and the eviction test queue several wrapper calls behind one filler and take one FILL_MS per call.
111 tests: 90 table rows through the delayed producer (eight of them added for tests/test_gpu_scratch.py, which reuses this table: scratch layouts no earlier
row reached), 12 interleaved groups, 9 further tests; 69 s for this file alone on the MI355X with 82 rows, 50 s of it the warm-up of every GPU session, so
about 20 s on top of the suite.

What this cannot see: inputs handed over as host arrays (geometry, delay tables, filters, weights); concurrent use of one plan from two streams without an
event between them, which the header does not promise."""
import collections
import contextlib
import ctypes as C
import os
import time

import numpy as np
import pytest
import torch

from tests import streams as ST
from tests.cases import make_case, rel_err
from tests.streams import same_bits

pytestmark = pytest.mark.gpu

FILL_MS = 16

# entry -> "file:line reason": the wrappers that wait for the stream.  Everything else must return while the filler is still running.
BLOCKS = {
    "hilbert": "qups_amd/preproc.py:hilbert -- torch.cuda.current_stream().synchronize() behind qdas_pre_execute, inside the plan's lock (its hipFFT work buffers are the plan's)",
    "eikonal": "qups_amd/csrc/eikonal.hip:269-270 -- the host reads the change counters back after every block of sweeps and ends the iteration (include/qdas.h: qdas_eikonal WAITS for the stream)",
    "das_lut": "qups_amd/csrc/das_lut.hip:263-307 -- the fused route probes the tables' fit per call: the misfit counter is read back (hipStreamSynchronize) before the frame launch",
    "adjoint": "qups_amd/adjoint.py:57 -- the bin selection: the spectrum's magnitudes come back to the host, which picks the frequency list",
    "shift_sum_first": "qups_amd/interpd.py:_shift_tables -- the first call per host table uploads it and synchronises the stream once, so that later hits may use the copies from any stream",
    "oneshot_das": "qups_amd/csrc/qdas_api.hip:one_shot -- a plan is created, executed and destroyed inside the call: it waits for the stream before the plan's tables are freed",
    "greens": "qups_amd/greens.py:38 -- every argument is a host array uploaded per call: a pageable upload on the caller's stream returns when the stream has reached it",
    "migration": "qups_amd/migration.py:103-104 -- tau and gamma are host arrays uploaded per call (a pageable upload on the caller's stream returns when the stream has reached it)",
    "migration_compose": "qups_amd/migration.py:129 -- the host tables of the composed path are uploaded per call, as above",
    "pwznxcorr": "qups_amd/correlator.py:222 -- the window weights are a host array uploaded per call, as above",
    "arena0": "qups_amd/csrc/scratch.hip:84-89 -- with QDAS_SCRATCH_ARENA_MAX_MB=0 every temporary is a per-call block, freed after a stream synchronisation when the call returns",
    "plan_close": "qups_amd/das_spec.py:DasPlan.close -- torch.cuda.synchronize(device) before qdas_plan_destroy: the documented wait",
}

CASES = collections.OrderedDict()            # case id -> (entry, exact, inter, builder)
SEEN = collections.OrderedDict()             # entry -> [cases run, cases that blocked]
HOST_MS = {}                                 # case id -> host wall time of a warm call on the default stream [ms]

# include/qdas.h prototype with a `void *stream` -> the case ids that reach it (tests/test_streams_host.py holds the header against this table)
HEADER = {
    "qdas_plan_execute": ["plan_execute_abi"],
    "qdas_plan_execute_frames": ["das-tiled-single", "das-generic-single", "das-frames2-prepared", "das-frames4-first", "das-frames4-twin-first"],
    "qdas_plan_delays": ["plan_delays-single", "plan_delays-double"],
    "qdas_fold": ["fold"],
    "qdas_plan_execute_sharded": ["sharded"],
    "qdas_DAS": ["oneshot-DAS"],
    "qdas_DASf": ["oneshot-DASf"],
    "qdas_DASh": ["oneshot-DASh"],
    "qdas_delays": ["oneshot-delays"],
    "qdas_delaysf": ["oneshot-delaysf"],
    "qdas_das_lut": ["das_lut-sum-single", "das_lut-sum-double", "das_lut-rx", "das_lut-tx", "das_lut-rxtx"],
    "qdas_wsinterpd": ["wsinterpd-lanesum", "wsinterpd-general", "wsinterpd-stream"],
    "qdas_greens": ["greens-single", "greens-double"],
    "qdas_shift_sum": ["shift_sum-host-tables", "shift_sum-device-tables"],
    "qdas_convd": ["convd-direct", "convd-fft", "convd-half"],
    "qdas_iir": ["sosfilt"],
    "qdas_coherence": ["coherence-average", "coherence-ensemble", "coherence-dmas", "coherence-cohfac", "coherence-pcf"],
    "qdas_eikonal": ["eikonal"],
    "qdas_eikonal_tables": ["eikonal_tables"],
    "qdas_adjoint": ["adjoint-sum", "adjoint-keep_tx", "adjoint-keep_rx"],
    "qdas_migration": ["migration-0", "migration-blocks", "migration-compose"],
    "qdas_pwznxcorr": ["pwznxcorr"],
    "qdas_permute3": ["permute3"],
    "qdas_pre_execute": ["hilbert-onepass", "hilbert-hipfft"],
}
EXEMPT = {}                                  # prototype -> reason (none today)


def case(cid, entry, exact=True, inter=None):
    """register a builder: a context manager that yields ``dict(fn=, tensors=[...], verify=None, ref_fn=None, warm=True)``.  ``inter``: the name of the
    interleaved group the case's call joins."""
    def deco(f):
        assert cid not in CASES
        CASES[cid] = (entry, exact, inter, contextlib.contextmanager(f))
        return f
    return deco


@pytest.fixture(scope="module")
def side():
    """two non-blocking streams kept for the whole module: the arenas of csrc/scratch.hip are per (device, stream)"""
    ST.calibrate()
    return torch.cuda.Stream(), torch.cuda.Stream()


def _np(t):
    return (t.to(torch.complex128) if t.is_complex() else t).cpu().numpy()


def _dev(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to("cuda", dt) if dt is not None else t.cuda()


# ================================================================================================================ DAS plans
def _mk_prob(cs, interp, prec, fun="DAS", xshape=None):
    from qups_amd import build_problem, parse_options
    xt = torch.from_numpy(cs["x"])
    po = parse_options(xt, list(cs["opt"]) + ["interp", interp, "input-precision", prec])
    return build_problem(fun, cs["Pi"], cs["Pr"], cs["Pv"], cs["Nv"], xshape or tuple(xt.shape), cs["t0"], cs["fs"], cs["c"], po)


def _das(cid, prec, kernel, inter=None):
    @case(cid, "das_plan", inter=inter)
    def _b():
        from tests import test_gpu_guards as TG
        plan, xc = TG._das_plan("FSA", "lanczos3", "DAS", prec, kernel)
        with plan:
            assert plan.kernel == ("tiled" if kernel == 2 else "generic")
            yield dict(fn=lambda x: plan.execute_colmajor(x, 1), tensors=[xc])


for _p in ("single", "halfT", "double"):
    _das(f"das-tiled-{_p}", _p, 2, inter="das" if _p == "single" else None)
    _das(f"das-generic-{_p}", _p, 1, inter="das" if _p != "halfT" else None)


@case("das-feval", "das_plan")
def _b():
    """``plan.feval``: the cast, the column-major copy (qdas_permute3) and the execute, all on the caller's stream"""
    from qups_amd import DasPlan
    cs = make_case(seq="PW", interp="cubic", seed=41, N=10, M=6, I1=203, I2=11)
    with DasPlan(_mk_prob(cs, "cubic", "single")) as plan:
        yield dict(fn=plan.feval, tensors=[torch.from_numpy(cs["x"]).cuda()])


def _fold_case():
    return make_case(seq="FSA", interp="lanczos3", seed=17, N=32, I1=150, I2=40)          # tests/test_gpu_mirror.py test_prefolded_plans_and_the_fold_entry


@case("das-folded", "das_plan", inter="das")
def _b():
    """a reciprocity-folded plan: the fold pass writes the plan's fold_buf, the fused kernel reads it"""
    from qups_amd import DasPlan
    from qups_amd.das_spec import _cast_data, _colmajor
    cs = _fold_case()
    with DasPlan(_mk_prob(cs, "lanczos3", "single"), kernel=2) as plan:
        assert plan.folded
        xc = _colmajor(_cast_data(torch.from_numpy(cs["x"]), "single", plan.device))
        yield dict(fn=lambda x: plan.execute_colmajor(x.reshape(1, *x.shape), 1), tensors=[xc])


@case("das-fp16-reciprocal", "das_plan")
def _b():
    """fp16 frames of a reciprocal problem: the parent plan folds into complex64 and hands the folded frame to its fp32 child"""
    from qups_amd import DasPlan
    from qups_amd.das_spec import _cast_data, _colmajor
    cs = _fold_case()
    with DasPlan(_mk_prob(cs, "lanczos3", "halfT"), kernel=2) as plan:
        assert plan.folded and plan.reciprocal
        xc = _colmajor(_cast_data(torch.from_numpy(cs["x"]), "halfT", plan.device))
        yield dict(fn=lambda x: plan.execute_colmajor(x.reshape(1, *x.shape), 1), tensors=[xc])


@case("das-split-aperture", "das_plan")
def _b():
    """tests/test_gpu_parity.py test_double_precision_aperture_split: several workgroups per tile, partial images, then the reduce"""
    from qups_amd import DasPlan
    from qups_amd.das_spec import _cast_data, _colmajor
    cs = make_case(seq="DV", interp="lanczos3", seed=8, N=24, I1=100, I2=21)
    old = os.environ.get("QDAS_KSPLIT")
    os.environ["QDAS_KSPLIT"] = "2"
    try:
        plan = DasPlan(_mk_prob(cs, "lanczos3", "double"), kernel=2)
    finally:
        if old is None:
            del os.environ["QDAS_KSPLIT"]
        else:
            os.environ["QDAS_KSPLIT"] = old
    with plan:
        assert plan.kernel == "tiled" and plan.aperture_split() == 2
        xc = _colmajor(_cast_data(torch.from_numpy(cs["x"]), "double", plan.device))
        yield dict(fn=lambda x: plan.execute_colmajor(x.reshape(1, *x.shape), 1), tensors=[xc])


def _kept(cid, fun):
    @case(cid, "das_plan", exact=False)
    def _b():
        """a kept aperture dimension on the fused kernel (float atomics into the planes): tests/test_gpu_guards.py's oracle and bound"""
        from tests import test_gpu_guards as TG
        plan, xc = TG._das_plan("PW", "lanczos3", fun, "single", 2)

        def verify(y):
            got, ref = TG._planes(y, TG._das_ref("PW", "lanczos3", fun, "single"))
            err = rel_err(got, ref)
            print(f"{cid}: rel_err={err:.3e}")
            assert err <= TG._das_tol("lanczos3", 2, "single", fun), err
        with plan:
            assert plan.kernel == "tiled"
            yield dict(fn=lambda x: plan.execute_colmajor(x, 1), tensors=[xc], verify=verify)


_kept("das-SYN", "SYN")
_kept("das-MUL", "MUL")


def _frames(cid, F, prepared):
    @case(cid, "das_plan")
    def _b():
        """a FRESH plan's first stream of F frames on the side stream (tests/test_gpu_mirror.py test_prepare_frames_ahead_of_the_first_stream): it memsets the second
        folded copy on the caller's stream and may build the twin; the serial reference comes from another plan of the same problem"""
        from qups_amd import DasPlan
        from qups_amd.das_spec import _colmajor
        cs = make_case(seq="FSA", interp="lanczos3", seed=29, N=32, I1=150, I2=40)
        rng = np.random.default_rng(3)
        xs = np.stack([cs["x"]] + [(rng.standard_normal(cs["x"].shape) + 1j * rng.standard_normal(cs["x"].shape)).astype(np.complex64) * 0.05 for _ in range(F - 1)], axis=3)
        prob = _mk_prob(cs, "lanczos3", "single", xshape=tuple(xs.shape))
        xc = _colmajor(torch.from_numpy(xs).cuda())
        with DasPlan(prob, kernel=2) as a, DasPlan(prob, kernel=2) as b:
            assert a.folded and b.folded
            if prepared:
                b.prepare_frames(F)
            yield dict(fn=lambda x: b.execute_colmajor(x, F), ref_fn=lambda x: a.execute_colmajor(x, F), tensors=[xc], warm=False,
                       frames=F, plan=b, fresh=lambda: DasPlan(prob, kernel=2))


for _F in (2, 4):
    _frames(f"das-frames{_F}-prepared", _F, True)
    _frames(f"das-frames{_F}-first", _F, False)          # (hipMalloc + hipMemsetAsync of the second folded copy on the caller's stream: nothing waits when the kernels exist)


def _frames_twin(cid, prepared):
    @case(cid, "das_plan")
    def _b():
        """tests/test_gpu_mirror.py test_mirror_mode_through_das_spec_and_frames: a general-mode lateral-mirror plan streams groups of four frames through a twin plan
        without the mode, created at the first such call -- here on the side stream, behind the delayed producer.  (qdas_plan_create works on the null stream and waits
        for that stream only: with the kernels at hand the call is back before the side stream has drained, which include/qdas.h allows but does not promise.)"""
        from qups_amd import DasPlan
        from qups_amd.das_spec import _colmajor
        cs = make_case(seq="PW", interp="cubic", seed=12, N=16, M=8, I1=80, I2=24)
        rng = np.random.default_rng(1)
        xs = np.stack([cs["x"]] + [(rng.standard_normal(cs["x"].shape) + 1j * rng.standard_normal(cs["x"].shape)).astype(np.complex64) for _ in range(3)], axis=3)
        prob = _mk_prob(cs, "cubic", "single", xshape=tuple(xs.shape))
        xc = _colmajor(torch.from_numpy(xs).cuda())
        with DasPlan(prob, kernel=2) as a, DasPlan(prob, kernel=2) as b:
            assert a.mirror and b.mirror and not a.reciprocal
            if prepared:
                b.prepare_frames(4)
            yield dict(fn=lambda x: b.execute_colmajor(x, 4), ref_fn=lambda x: a.execute_colmajor(x, 4), tensors=[xc], warm=False,
                       frames=4, plan=b, fresh=lambda: DasPlan(prob, kernel=2))


_frames_twin("das-frames4-twin-prepared", True)
_frames_twin("das-frames4-twin-first", False)


@case("das-mirror", "das_plan")
def _b():
    """ONE frame through a general-mode lateral-mirror plan (the frames4-twin rows above send theirs through the twin, which has no mirror mode): two window
    sets, and -- few tiles -- a split aperture whose partial images hold both halves of the image"""
    from qups_amd import DasPlan
    from qups_amd.das_spec import _colmajor
    cs = make_case(seq="PW", interp="cubic", seed=12, N=16, M=8, I1=80, I2=24)
    with DasPlan(_mk_prob(cs, "cubic", "single"), kernel=2) as plan:
        assert plan.kernel == "tiled" and plan.mirror and not plan.reciprocal
        xc = _colmajor(torch.from_numpy(cs["x"]).cuda())
        yield dict(fn=lambda x: plan.execute_colmajor(x.reshape(1, *x.shape), 1), tensors=[xc])


@case("das-misfit", "das_plan")
def _b():
    """tests/test_gpu_parity.py test_oversize_window_falls_back: 49 samples of delay per pixel -- tiles that fit no window are listed by the fused kernel in the
    plan's fallback list and redone by the generic kernel behind it (and behind the reduce of the split aperture, which reads their unwritten partial images)"""
    from qups_amd import DasPlan
    from qups_amd.das_spec import _cast_data, _colmajor
    cs = make_case(seq="PW", interp="cubic", seed=16, I1=60, I2=6, zlim=(2e-3, 120e-3), data="noise", N=8, M=4)
    with DasPlan(_mk_prob(cs, "cubic", "single"), kernel=0) as plan:
        xc = _colmajor(_cast_data(torch.from_numpy(cs["x"]), "single", plan.device))
        fn = lambda x: plan.execute_colmajor(x.reshape(1, *x.shape), 1)
        fn(xc)
        torch.cuda.synchronize()                               # (fallback_tiles reads the count the last frame left in the list)
        assert plan.kernel == "tiled" and plan.fallback_tiles() > 0 and plan.aperture_split() > 1, (plan.kernel, plan.fallback_tiles(), plan.aperture_split())
        yield dict(fn=fn, tensors=[xc])


@case("plan_execute_abi", "das_plan")
def _b():
    """qdas_plan_execute itself (the wrappers go through qdas_plan_execute_frames)"""
    from qups_amd import _lib
    from tests import test_gpu_guards as TG
    plan, xc = TG._das_plan("PW", "lanczos3", "DAS", "single", 0)
    L = _lib.lib()

    def fn(x):
        y = torch.empty((1, 1, 1, plan.out_count), dtype=torch.complex64, device="cuda")
        _lib.check(L.qdas_plan_execute(plan._h, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return y
    with plan:
        yield dict(fn=fn, tensors=[xc])


def _delays(prec):
    @case(f"plan_delays-{prec}", "das_plan_delays")
    def _b():
        from tests import test_gpu_guards as TG
        plan, _ = TG._das_plan("PW", "lanczos3", "DAS", prec, 0)
        with plan:
            yield dict(fn=plan.delays, tensors=[])


_delays("single")
_delays("double")


@case("fold", "fold")
def _b():
    from qups_amd import _lib
    from qups_amd.das_spec import _colmajor
    cs = _fold_case()
    T, N, M = cs["x"].shape
    xc = _colmajor(torch.from_numpy(cs["x"]).cuda())
    d = _lib.FoldDesc(T, N, 0, 0, 1, -1, None)

    def fn(x):
        xs = torch.zeros((M, N, T), dtype=torch.complex64, device="cuda")
        _lib.check(_lib.lib().qdas_fold(C.byref(d), C.c_void_p(x.data_ptr()), C.c_void_p(xs.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return xs
    yield dict(fn=fn, tensors=[xc])


@case("permute3", "permute3")
def _b():
    from qups_amd.das_spec import _colmajor
    t = torch.randn((65, 3, 33), device="cuda", generator=torch.Generator(device="cuda").manual_seed(101))
    yield dict(fn=_colmajor, tensors=[t])


def _oneshot(name):
    @case(f"oneshot-{name}", "oneshot_delays" if name.startswith("delays") else "oneshot_das")
    def _b():
        """tests/test_gpu_parity.py test_c_abi_one_shot_matches_plan: the reference kernels' own argument lists, every array a device pointer"""
        from qups_amd import _lib
        from qups_amd.das_spec import _cast_data
        dbl, half, delays = name in ("DAS", "delays"), name == "DASh", name.startswith("delays")
        cs = make_case(seq="PW", interp="linear", seed=19, N=6, M=3, I1=40, I2=4)
        prec = "double" if dbl else ("halfT" if half else "single")
        p = _mk_prob(cs, "linear", prec)
        L = _lib.lib()
        rt = torch.float64 if dbl else torch.float32
        geo = [_dev(a, rt) for a in (p.Pi, p.Pr, p.Pv, p.Nv, p.cinv)]
        xc = _cast_data(torch.from_numpy(cs["x"]), prec, torch.device("cuda", torch.cuda.current_device())).permute(2, 1, 0).contiguous()
        sz = _lib.Sizes(p.T, p.N, p.M, p.Isz[0], p.Isz[1], p.Isz[2], 0, p.flag, int(p.VS), int(p.DV), {"double": 0, "single": 1, "halfT": 2}[prec])
        assert sz.dtype == __import__("qups_amd.das_spec", fromlist=["_PREC"])._PREC[prec]
        acs = (C.c_uint64 * 6)(*[0] * 6)
        tv = ((C.c_double if dbl else C.c_float) * 2)(p.fs, 0.0)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        cinv0 = float(p.cinv.reshape(-1)[0])

        def fn(x, Pi, Pr, Pv, Nv, cinv):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            if delays:
                tau = torch.empty((p.M, p.N, p.I), dtype=rt, device="cuda")
                _lib.check(getattr(L, "qdas_" + name)(C.byref(sz), ptr(tau), ptr(Pi), ptr(Pr), ptr(Pv), ptr(Nv), cinv0, st))
                return tau
            y = torch.empty(p.I, dtype=x.dtype, device="cuda")
            _lib.check(getattr(L, "qdas_" + name)(C.byref(sz), ptr(y), ptr(Pi), ptr(Pr), ptr(Pv), ptr(Nv), None, ptr(cinv), acs, ptr(x), C.cast(tv, C.c_void_p), st))
            return y
        yield dict(fn=fn, tensors=[xc] + geo)


for _n in ("DAS", "DASf", "DASh", "delays", "delaysf"):
    _oneshot(_n)


@case("sharded", "sharded")
def _b():
    """tests/test_gpu_parity.py test_sharded_c_abi_entry_on_one_device: a repeated ordinal, every shard on device 0"""
    from qups_amd import MultiDevicePlan
    cs = make_case(seq="PW", interp="cubic", seed=41, N=10, M=6, I1=203, I2=11)
    mp = MultiDevicePlan(_mk_prob(cs, "cubic", "single"), devices=[0, 0])
    try:
        yield dict(fn=mp.feval, tensors=[torch.from_numpy(cs["x"]).cuda()])
    finally:
        mp.close()


# ================================================================================================================ das_lut, wsinterpd, shift_sum
def _lut(cid, keep_rx, keep_tx, prec, inter=None):
    fused = prec == "single" and not (keep_rx and keep_tx)           # fp32 data, at most one kept dimension: the table-driven fused kernel
    @case(cid, "das_lut" if fused else "das_lut_generic", exact=not (keep_rx or keep_tx), inter=inter)
    def _b():
        from oracle import das_oracle as O
        from qups_amd.interpd import das_lut
        from tests import test_gpu_guards as TG
        cs, tau_rx, tau_tx = TG._lut_case()
        fs, t0 = cs["fs"], cs["t0"]
        rt, ct = (torch.float64, torch.complex128) if prec == "double" else (torch.float32, torch.complex64)
        x, n1, n2 = _dev(cs["x"], ct), _dev(tau_rx * fs, rt), _dev((tau_tx - t0) * fs, rt)

        def fn(xx, a, b):
            y = das_lut(xx, a, b, interp="cubic", keep_rx=keep_rx, keep_tx=keep_tx, prec=prec)
            fn.kernel = das_lut.last_kernel
            return y

        def verify(y):                                           # tests/test_gpu_guards.py test_das_lut_outputs: 1e-9 (double), 5e-4 (single)
            ref = O.das_lut(cs["x"], tau_rx, tau_tx, t0, fs, interp="cubic", keep_rx=keep_rx, keep_tx=keep_tx)
            assert rel_err(_np(y).reshape(ref.shape), ref) <= (1e-9 if prec == "double" else 5e-4)
        yield dict(fn=fn, tensors=[x, n1, n2], verify=verify, route="tiled" if fused else "generic")


_lut("das_lut-sum-single", False, False, "single", inter="das_lut")          # the table-driven fused route
_lut("das_lut-sum-double", False, False, "double", inter="das_lut")          # the generic route
_lut("das_lut-rx", True, False, "single", inter="das_lut")
_lut("das_lut-tx", False, True, "single", inter="das_lut")
_lut("das_lut-rxtx", True, True, "single")


def lut_mirror_tables(a_rx, a_tx, lat, I1=140, I2=40, N=32, M=32):
    """synthetic split-delay tables in SAMPLES (float32, I1 x I2 x N and I1 x I2 x M) that are their own lateral mirror images: a depth slope ``a * i1``, a
    lateral term ``lat * column`` and a small offset per element in the first half of the columns; the second half is the exact mirror image of the first
    (tests/test_gpu_golden.py test_das_lut_mirror_symmetric_tables_take_the_mirror_mode).  Inside a tile of R rows and C columns every element's delays
    spread over ``a (R - 1) + lat (C - 1)`` samples: what the window-fit rule of csrc/tile_prologue.h sees."""
    assert I2 % 2 == 0
    i1, c = np.arange(I1, dtype=np.float64)[:, None, None], np.arange(I2, dtype=np.float64)[None, :, None]
    mk = lambda a, E: (4.0 + a * i1 + lat * c + 0.03 * np.arange(E, dtype=np.float64)[None, None, :]).astype(np.float32)
    rx, tx = mk(a_rx, N), mk(a_tx, M)
    h = I2 // 2
    rx[:, -h:, :] = rx[:, :h, :][:, ::-1, ::-1]
    tx[:, -h:, :] = tx[:, :h, :][:, ::-1, ::-1]
    return rx, tx


def lut_mirror_data(T=1024, N=32, M=32):
    rng = np.random.default_rng(61)
    return (rng.standard_normal((T, N, M)) + 1j * rng.standard_normal((T, N, M))).astype(np.complex64)


@case("das_lut-mirror", "das_lut")
def _b():
    """the mirror build of qdas_das_lut (fp32, full sum, no weights, kM >= 32; exists as a hiprtc build only): 6 tiles of the half image, so eight workgroups per
    tile and partial images (ks2 = 8) from the arena behind the misfit counter and the symmetry flag"""
    from qups_amd.interpd import das_lut
    rx, tx = lut_mirror_tables(0.5, 0.5, 0.05)
    x, n1, n2 = _dev(lut_mirror_data()), _dev(rx), _dev(tx)

    def fn(xx, a, b):
        y = das_lut(xx, a, b, interp="cubic", prec="single")
        fn.kernel = das_lut.last_kernel
        return y
    fn(x, n1, n2)
    torch.cuda.synchronize()
    if "mirror" not in fn.kernel:                              # (no hiprtc on this box: the mode exists as a specialised build only)
        pytest.skip("no mirror build: " + fn.kernel)
    yield dict(fn=fn, tensors=[x, n1, n2], route="tiled,mirror")


def _ws(cid, M, sdim):
    @case(cid, "wsinterpd", inter="wsinterpd")
    def _b():
        from qups_amd.interpd import wsinterpd
        from tests import test_gpu_guards as TG
        xs, ts, w, wa = TG._ws_case("single", M, "real")
        yield dict(fn=lambda x, t, ww: wsinterpd(x, t, 1, ww, sdim, "lanczos3", 0.0, 0.13j, prec="single"),
                   tensors=[_dev(xs, torch.complex64), _dev(ts, torch.float32), wa.cuda()])


_ws("wsinterpd-lanesum", 33, [3])              # one summed dimension of >= 16 terms
_ws("wsinterpd-general", 12, [3])              # the strided general kernel on the transposed copies
_ws("wsinterpd-stream", 33, None)              # nothing summed: one output per lane
_ws("wsinterpd-general-31", 31, [2])


def _shift(cid, host_tables):
    @case(cid, "shift_sum", inter="shift_sum" if host_tables else None)
    def _b():
        from qups_amd.interpd import shift_sum
        from tests import test_gpu_guards as TG
        x, shift, w, pad = TG._shift_case("complex64")
        T = x.shape[0]
        if host_tables:
            yield dict(fn=lambda xx: shift_sum(xx, shift, w, "cubic", To=T + 17, tpad=pad), tensors=[_dev(x)])
        else:
            yield dict(fn=lambda xx, s, ww: shift_sum(xx, s, ww, "cubic", To=T + 17, tpad=pad), tensors=[_dev(x), _dev(shift), _dev(w)])


@case("shift_sum-first-table", "shift_sum_first")
def _b():
    """the first call with a host table (the memo is emptied in front of every call): it uploads the table and synchronises the stream once"""
    from qups_amd import interpd
    from tests import test_gpu_guards as TG
    x, shift, w, pad = TG._shift_case("complex64")

    def fn(xx):
        with interpd._SHIFT_MEMO_LOCK:
            if interpd._SHIFT_MEMO is not None:
                interpd._SHIFT_MEMO.clear()
        return interpd.shift_sum(xx, shift, w, "cubic", To=x.shape[0] + 17, tpad=pad)
    yield dict(fn=fn, tensors=[_dev(x)])


_shift("shift_sum-host-tables", True)          # a memo hit after the warm calls: no wait
_shift("shift_sum-device-tables", False)


def _shift64(cid, weights):
    @case(cid, "shift_sum")
    def _b():
        """fp64 data: table entries of 56 instead of 28 bytes in the stream's arena, with and without a weight table"""
        from qups_amd.interpd import shift_sum
        from tests import test_gpu_guards as TG
        x, shift, w, pad = TG._shift_case("complex128")
        T = x.shape[0]
        if weights:
            yield dict(fn=lambda xx, s, ww: shift_sum(xx, s, ww, "cubic", To=T + 17, tpad=pad), tensors=[_dev(x), _dev(shift), _dev(w)])
        else:
            yield dict(fn=lambda xx, s: shift_sum(xx, s, None, "cubic", To=T + 17, tpad=pad), tensors=[_dev(x), _dev(shift)])


_shift64("shift_sum-double", True)
_shift64("shift_sum-double-noweights", False)


# ================================================================================================================ greens, convd, iir, hilbert
def _greens(prec):
    @case(f"greens-{prec}", "greens", inter="greens")
    def _b():
        """every argument is a host array that the wrapper uploads itself: no producer to delay; the consumer and the interleaving remain"""
        from qups_amd.greens import greens_kernel
        from tests.test_greens import _setup
        g = _setup(seed=5, N=9, M=7, I=40, En=2, Em=3, fsr=1.0)
        args = (g["Ps"], g["a"], g["Pr"], g["Pv"], g["x"], g["S"], g["s0"], g["t0"], g["fs"], 1.0, g["cinv"], g["R0"], "linear")
        yield dict(fn=lambda: greens_kernel(*args, prec), tensors=[])


_greens("single")
_greens("double")


def _greens_trains(cid, I):
    @case(cid, "greens")
    def _b():
        """the impulse-train kernels (QDAS_GREENS_TRAIN_MIN=0, read per call): distance tables, chunk bounds, tap list in the stream's arena -- and, from 4096
        scatterers on, the Morton sort's keys, histogram and sorted copies.  The trains are integer sums: bit-reproducible."""
        from qups_amd.greens import greens_kernel
        from tests.test_greens import _setup
        g = _setup(seed=5, N=9, M=7, I=I, En=2, Em=3, fsr=1.0)
        args = (g["Ps"], g["a"], g["Pr"], g["Pv"], g["x"], g["S"], g["s0"], g["t0"], g["fs"], 1.0, g["cinv"], g["R0"], "linear")

        def fn(train_min="0"):
            old = os.environ.get("QDAS_GREENS_TRAIN_MIN")
            os.environ["QDAS_GREENS_TRAIN_MIN"] = train_min
            try:
                return greens_kernel(*args, "single")
            finally:
                if old is None:
                    del os.environ["QDAS_GREENS_TRAIN_MIN"]
                else:
                    os.environ["QDAS_GREENS_TRAIN_MIN"] = old
        yield dict(fn=fn, tensors=[])


_greens_trains("greens-trains", 300)                  # two chunks of 256 scatterers, the second ragged; no sort
_greens_trains("greens-trains-sorted", 4100)          # the sort / gather pass (>= 4096 scatterers), 17 chunks, the last ragged


@case("convd-direct", "convd", inter="convd")
def _b():
    from qups_amd import convd
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((301, 70)) + 1j * rng.standard_normal((301, 70))).astype(np.complex64)
    k = (rng.standard_normal((37, 70)) + 1j * rng.standard_normal((37, 70))).astype(np.complex64)
    yield dict(fn=lambda a, b: convd(a, b, 1, "same"), tensors=[_dev(x), _dev(k)])


@case("convd-fft", "convd", inter="convd")
def _b():
    """tests/test_convd.py test_convd_long_filters_take_the_fft_path: 129 taps, the filter spectrum and twiddles in the stream's arena"""
    from qups_amd import convd
    rng = np.random.default_rng(829)
    x = (rng.standard_normal((37, 700)) + 1j * rng.standard_normal((37, 700))).astype(np.complex64)
    h = (rng.standard_normal(129) * np.hanning(129)).astype(np.float32)

    def fn(a, b):
        old = os.environ.get("QDAS_CONV_FFT_MIN_TAPS")
        os.environ["QDAS_CONV_FFT_MIN_TAPS"] = "90"
        try:
            return convd(a, b, 2, "full")
        finally:
            if old is None:
                del os.environ["QDAS_CONV_FFT_MIN_TAPS"]
            else:
                os.environ["QDAS_CONV_FFT_MIN_TAPS"] = old
    yield dict(fn=fn, tensors=[_dev(x), _dev(h).reshape(1, 129)])


@case("convd-half", "convd", inter="convd")
def _b():
    from qups_amd import convd
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((1500, 3, 2)) * 0.25).astype(np.float16)
    k = (rng.standard_normal((37, 1, 1)) * 0.25).astype(np.float16)
    yield dict(fn=lambda a, b: convd(a, b, 1, "same"), tensors=[_dev(x), _dev(k)])


@case("convd-direct-2", "convd", inter="convd")
def _b():
    from qups_amd import convd
    rng = np.random.default_rng(6)
    x = rng.standard_normal((3, 129, 5)).astype(np.float32)
    k = rng.standard_normal((1, 9, 1)).astype(np.float32)
    yield dict(fn=lambda a, b: convd(a, b, 2, "full"), tensors=[_dev(x), _dev(k)])


@case("sosfilt", "iir")
def _b():
    from scipy import signal
    from qups_amd import sosfilt
    rng = np.random.default_rng(7)
    x = (rng.standard_normal((301, 70)) + 1j * rng.standard_normal((301, 70))).astype(np.complex64)
    sos = signal.butter(4, [0.1, 0.4], "band", output="sos")
    yield dict(fn=lambda a: sosfilt(a, sos, 1, 1.0), tensors=[_dev(x)])


def _hilbert(cid, T, N, K, force):
    @case(cid, "hilbert", inter="hilbert-hipfft" if force else "hilbert")
    def _b():
        from qups_amd.preproc import hilbert
        x = np.random.default_rng(T + K).standard_normal((T, K)).astype(np.float32)

        def fn(a):
            old = os.environ.get("QDAS_PRE_HIPFFT")
            os.environ["QDAS_PRE_HIPFFT"] = "1" if force else "0"
            try:
                y = hilbert(a, N)
                assert hilbert.last_one_pass == (not force)
                return y
            finally:
                if old is None:
                    del os.environ["QDAS_PRE_HIPFFT"]
                else:
                    os.environ["QDAS_PRE_HIPFFT"] = old
        yield dict(fn=fn, tensors=[_dev(x)])


_hilbert("hilbert-onepass", 300, 512, 5, False)
_hilbert("hilbert-hipfft", 300, 512, 5, True)          # plan-owned work buffers
for _k, (_T, _N, _K) in enumerate([(2816, None, 7), (256, None, 3), (1000, None, 3)]):
    _hilbert(f"hilbert-onepass-{_k}", _T, _N, _K, False)
    _hilbert(f"hilbert-hipfft-{_k}", 300, 512, 5, True)          # the SAME shape on both streams: one plan, its buffers shared


# ================================================================================================================ coherence, eikonal, adjoint, migration, pwznxcorr
def _coh(method):
    @case(f"coherence-{method}", "coherence", inter="coherence" if method != "pcf" else None)
    def _b():
        from tests import test_gpu_coherence as H
        x = H._data((37, 3, 7), True, seed=sum(map(ord, method)), zero_px=True)
        xt = H._layout(x, torch.complex64, "odd")          # a strided view: the skipped rows are poison too
        yield dict(fn=lambda a: H._run(method, a, 3), tensors=[xt])


for _m in ("average", "ensemble", "dmas", "cohfac", "pcf"):
    _coh(_m)


@case("eikonal", "eikonal", inter="eikonal")
def _b():
    from tests import eikonal_ref as R
    from tests import test_gpu_eikonal as H
    c = R.smooth_random(17, 33, seed=17 + 3300)
    sets = [[[1.0], [1.0]], [[17.0], [33.0]]]
    yield dict(fn=lambda cc: H._solve(cc, H.DP, sets).contiguous(), tensors=[_dev(c)])


@case("eikonal-chunks", "eikonal")
def _b():
    """a map of 3 x 5 tiles: the fronts need more passes than one chunk of four (csrc/eikonal.hip CHUNK), so the chunk's counters are cleared and reused"""
    from qups_amd import eikonal as E
    from tests import eikonal_ref as R
    from tests import test_gpu_eikonal as H
    c = R.smooth_random(40, 70, seed=40 + 7000)
    sets = [[[1.0], [1.0]], [[40.0], [70.0]]]

    def fn(cc):
        T = H._solve(cc, H.DP, sets).contiguous()
        assert E.last_passes() > 4, E.last_passes()
        return T
    yield dict(fn=fn, tensors=[_dev(c)])


def _eik_tables(cid, npix, inter):
    @case(cid, "eikonal_tables", inter=inter)
    def _b():
        from qups_amd import eikonal as E
        from tests import eikonal_ref as R
        from tests import test_gpu_eikonal as H
        C1, C2, K = 17, 33, 3
        c = R.smooth_random(C1, C2, seed=C1 + 100 * C2)
        src = np.array([[1.0, 9.3, 17.0], [1.0, 20.1, 33.0]])
        Tm = H._solve(c, H.DP, [src[:, k:k + 1] for k in range(K)])          # (a C1 x C2 x K view of K x C2 x C1 storage: read where it lies)
        rng = np.random.default_rng(3)
        Pi = np.stack([rng.uniform(0.2, C1 + 0.8, npix), rng.uniform(0.2, C2 + 0.8, npix)])
        yield dict(fn=lambda Th, Ph: E.eikonal_tables(Th, Ph).contiguous(), tensors=[Tm, _dev(Pi)])


_eik_tables("eikonal_tables", 75, "eikonal")
_eik_tables("eikonal_tables-300", 300, "eikonal")
_eik_tables("eikonal_tables-9", 9, "eikonal")


def _adjoint(cid, **kw):
    @case(cid, "adjoint", inter="adjoint")
    def _b():
        """the core shape of tests/test_gpu_adjoint.py; pixel blocks (QDAS_ADJOINT_BLOCK_BYTES) make the summed image a reduce of partial images"""
        from qups_amd import ChannelData
        from tests import test_gpu_adjoint as H
        us = H._system("PW", 20, 7, 37, 5)
        x, t0 = H._data(96, 20, 7, seed=1)
        block = kw.pop("block", None)

        def fn(xx):
            old = os.environ.get("QDAS_ADJOINT_BLOCK_BYTES")
            if block:
                os.environ["QDAS_ADJOINT_BLOCK_BYTES"] = block
            try:
                return us.bfAdjoint(ChannelData(xx, t0, H.FS), fmod=2.5e6, **kw)
            finally:
                if block:
                    if old is None:
                        del os.environ["QDAS_ADJOINT_BLOCK_BYTES"]
                    else:
                        os.environ["QDAS_ADJOINT_BLOCK_BYTES"] = old
        yield dict(fn=fn, tensors=[_dev(x)])


_adjoint("adjoint-sum")
_adjoint("adjoint-sum-blocks", block="20000")
_adjoint("adjoint-keep_tx", keep_tx=True)
_adjoint("adjoint-keep_rx", keep_rx=True)


def _migration(cid, which, keep_tx=False, per_block=None, compose=False, inter="migration"):
    @case(cid, "migration_compose" if compose else "migration", inter=inter)
    def _b():
        from qups_amd import migration as MG
        from tests import test_gpu_migration as H
        T, N, M, nfft = H.ODD if compose else ((64, 16, 5, None) if per_block else H.SHAPES[which])
        x, tau, gam = H._data(T, N, M)

        def fn(xx):
            if compose:
                return MG.compose(xx, H.T0, H.FS, tau, gam, H.PITCH, H.C0, nfft)
            old = os.environ.get("QDAS_MIGRATION_BLOCK_BYTES")
            if per_block:
                os.environ["QDAS_MIGRATION_BLOCK_BYTES"] = str(per_block * 64 * 16 * 8)
            try:
                return MG.migrate(xx, H.T0, H.FS, tau, gam, H.PITCH, H.C0, nfft, 0.0, "cubic", True, keep_tx)
            finally:
                if per_block:
                    if old is None:
                        del os.environ["QDAS_MIGRATION_BLOCK_BYTES"]
                    else:
                        os.environ["QDAS_MIGRATION_BLOCK_BYTES"] = old
        yield dict(fn=fn, tensors=[_dev(x)])


for _w in range(4):
    _migration(f"migration-{_w}", _w)
_migration("migration-blocks", None, per_block=2)
_migration("migration-blocks-keep_tx", None, keep_tx=True, per_block=2, inter=None)
_migration("migration-compose", None, compose=True, inter=None)


@case("pwznxcorr", "pwznxcorr")
def _b():
    from qups_amd import pwznxcorr
    from tests import test_gpu_pwznxcorr as P
    xt = P._colmajor(P._data((96, 5), True, seed=7), torch.complex64)
    yield dict(fn=lambda a: pwznxcorr(a, 3, 7), tensors=[xt])


# ================================================================================================================ the arena's per-call paths
def _arena0(cid, base):
    entry, exact, _, builder = CASES[base]

    @case(cid, "arena0", exact=exact)
    def _b():
        """the same call with QDAS_SCRATCH_ARENA_MAX_MB=0 (read per call): every temporary is a block of its own (the ``big_`` path of csrc/scratch.hip)"""
        with builder() as c:
            inner = c["fn"]

            def fn(*a):
                os.environ["QDAS_SCRATCH_ARENA_MAX_MB"] = "0"
                try:
                    return inner(*a)
                finally:
                    del os.environ["QDAS_SCRATCH_ARENA_MAX_MB"]
            c = dict(c, fn=fn)
            c.pop("route", None)
            yield c


_arena0("arena0-shift_sum", "shift_sum-device-tables")
_arena0("arena0-das_lut", "das_lut-sum-single")
_arena0("arena0-convd-fft", "convd-fft")
_arena0("arena0-migration", "migration-1")
_arena0("arena0-greens", "greens-single")


# ================================================================================================================ the table, run
def _time_host(fn, tensors):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn(*tensors)
    ms = (time.perf_counter() - t) * 1e3
    torch.cuda.synchronize()
    return r, ms


def _check_case(cid, side_stream, ms=FILL_MS, blocks=BLOCKS):
    """steps 1-4 of the module docstring for one row; returns whether the wrapper returned early"""
    entry, exact, _, builder = CASES[cid]
    with builder() as c:
        fn, tensors, verify = c["fn"], c["tensors"], c.get("verify")
        ref_fn = c.get("ref_fn") or fn
        r0 = ST._tup(ref_fn(*tensors))
        torch.cuda.synchronize()
        r1, host_ms = _time_host(ref_fn, tensors)
        r1 = ST._tup(r1)
        HOST_MS[cid] = host_ms
        if exact:
            assert all(same_bits(a, b) for a, b in zip(r0, r1)), f"{cid}: two serial runs on the default stream differ"
        if "route" in c:
            assert fn.kernel.startswith(c["route"]), (cid, fn.kernel)
        if c.get("warm", True):
            with torch.cuda.stream(side_stream):
                fn(*tensors)
                fn(*tensors)
            torch.cuda.synchronize()
        outs, clones, early = ST.run_delayed(fn, tensors, side_stream, ms)
        for what, got in (("output", outs), ("clone taken on the stream behind the call", clones)):
            assert len(got) == len(r0), (cid, what)
            if exact:
                bad = [k for k, (a, b) in enumerate(zip(got, r0)) if not same_bits(a, b)]
                assert not bad, f"{cid}: the {what} on a side stream behind a delayed producer differs from the serial result (an internal step is not ordered on the caller's stream)"
            else:
                verify(got[0] if len(got) == 1 else got)
    s = SEEN.setdefault(entry, [0, 0])
    s[0] += 1
    s[1] += not early
    print(f"streams: {cid:28s} entry={entry:18s} host_ms={host_ms:7.3f} early={early}")
    if os.environ.get("QDAS_STREAMS_MEASURE"):                  # (a measuring run reports every case before any early-return assertion)
        return early
    if entry in blocks:
        assert not early, f"{cid}: BLOCKS lists '{entry}' ({blocks[entry]}) but the wrapper returned while the filler was still running: the table must stay true"
    else:
        assert early, f"{cid}: the wrapper did not return before {ms} ms of queued work had run, and '{entry}' is not in BLOCKS: it waits for the stream (or for the device)"
    return early


@pytest.mark.parametrize("cid", list(CASES))
def test_delayed_producer_and_consumer(cid, side):
    _check_case(cid, side[0])


GROUPS = collections.OrderedDict()
for _cid, (_e, _x, _g, _b) in CASES.items():
    if _g:
        GROUPS.setdefault(_g, []).append(_cid)


@pytest.mark.parametrize("group", list(GROUPS))
def test_interleaved_on_two_streams(group, side):
    """the group's calls (padded to at least four by repeating them with their own fresh inputs) issued alternately on two streams"""
    ids = GROUPS[group]
    while len(ids) < 4:
        ids = ids + GROUPS[group]
    with contextlib.ExitStack() as es:
        calls, checks = [], []
        for cid in ids:
            c = es.enter_context(CASES[cid][3]())
            calls.append((lambda c=c: c["fn"](*c["tensors"])))
            checks.append(None if CASES[cid][1] else c["verify"])          # (float atomics: the home file's parity check instead of bit equality)
        ST.interleaved(calls, side[0], side[1], FILL_MS * len(calls), checks=checks)          # (one FILL_MS per queued call: nothing runs until all are queued)
    SEEN.setdefault("interleaved", [0, 0])[0] += 1


# ================================================================================================================ further cases
def test_one_plan_handed_from_one_stream_to_the_next(side):
    """frame A on s1, ``s2.wait_stream(s1)``, frame B on s2: the legitimate hand-off; what the plan owns (fold buffer, fallback-tile list) carries over"""
    from qups_amd import DasPlan
    from qups_amd.das_spec import _colmajor
    s1, s2 = side
    cs = _fold_case()
    xa = _colmajor(torch.from_numpy(cs["x"]).cuda())
    xb = (xa * (0.5 - 0.25j)).flip(2).contiguous()
    with DasPlan(_mk_prob(cs, "lanczos3", "single"), kernel=2) as plan:
        assert plan.folded
        run = lambda x: plan.execute_colmajor(x.reshape(1, *x.shape), 1)
        ra, rb = run(xa), run(xb)
        torch.cuda.synchronize()
        (ta, tb), _ = ST.delayed(s1, [xa, xb], FILL_MS)
        with torch.cuda.stream(s1):
            ya = run(ta)
        s2.wait_stream(s1)
        with torch.cuda.stream(s2):
            yb = run(tb)
            cb = yb.clone()
        torch.cuda.synchronize()
        assert same_bits(ya, ra) and same_bits(yb, rb) and same_bits(cb, rb)
    SEEN.setdefault("das_plan_handoff", [0, 0])[0] += 1


def test_pipeline_on_two_streams(side):
    """greens -> real RF -> hilbert (s1) -> convd band-pass (s1) -> ``s2.wait_stream(s1)`` -> DAS (s2) with the sizes of tests/test_preproc.py
    test_real_rf_hilbert_then_das_equals_das_of_the_analytic_data: bit-equal to the same chain on the default stream"""
    from scipy.signal import firwin
    from qups_amd import DasPlan, convd
    from qups_amd.greens import greens_kernel
    from qups_amd.das_spec import _colmajor
    from qups_amd.preproc import hilbert
    from tests.test_greens import _setup
    s1, s2 = side
    cs = make_case(seq="PW", interp="cubic", seed=95, N=16, I1=120, I2=16, zlim=(4e-3, 14e-3), xspan=3e-3)
    T, N, M = cs["x"].shape
    g = _setup(seed=5, N=N, M=M, I=40, En=1, Em=1, fsr=1.0)
    args = (g["Ps"], g["a"], g["Pr"], g["Pv"], g["x"], g["S"], g["s0"], g["t0"], g["fs"], 1.0, g["cinv"], g["R0"], "linear")
    taps = _dev(firwin(25, [0.1, 0.6], pass_zero=False).astype(np.float32)).reshape(25, 1, 1)
    noise = _dev(cs["x"].real.astype(np.float32))
    with DasPlan(_mk_prob(cs, "cubic", "single"), kernel=0) as plan:
        def chain(sa, sb):
            with torch.cuda.stream(sa):
                sim = greens_kernel(*args, "single")                                   # S x N x M complex: what a simulation delivers
                rf = torch.zeros((T, N, M), dtype=torch.float32, device="cuda")
                n = min(T, sim.shape[0])
                rf[:n] = sim.real[:n] + noise[:n]
                xa = hilbert(rf)
                xf = convd(xa, taps.to(xa.dtype), 1, "same")
                xc = _colmajor(xf.contiguous())
            sb.wait_stream(sa)
            with torch.cuda.stream(sb):
                y = plan.execute_colmajor(xc.reshape(1, *xc.shape), 1)
                return y, y.clone(), xc
        d = torch.cuda.default_stream()
        y0, _, _ = chain(d, d)
        torch.cuda.synchronize()
        ST.filler(s1, FILL_MS)
        y1, c1, keep = chain(s1, s2)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(torch.view_as_real(y0)).all()) and float(y0.abs().max()) > 0
        assert same_bits(y1, y0) and same_bits(c1, y0)
    SEEN.setdefault("pipeline", [0, 0])[0] += 1


def test_close_right_after_an_execute_queued_behind_a_filler(side):
    """``plan.close()`` waits for work already queued on the device (its tables must outlive the launches that read them): the image is right, and close blocked"""
    from tests import test_gpu_guards as TG
    plan, xc = TG._das_plan("FSA", "lanczos3", "DAS", "single", 2)
    ref = plan.execute_colmajor(xc, 1)
    torch.cuda.synchronize()
    (tw,), ev = ST.delayed(side[0], [xc], FILL_MS)
    with torch.cuda.stream(side[0]):
        y = plan.execute_colmajor(tw, 1)
        queued = ST.returned_early(ev)
        plan.close()
        after = ST.returned_early(ev)
    torch.cuda.synchronize()
    assert same_bits(y, ref)
    assert queued and not after, (queued, after, BLOCKS["plan_close"])
    s = SEEN.setdefault("plan_close", [0, 0])
    s[0] += 1
    s[1] += 1


def test_arenas_regrow_on_each_of_two_fresh_streams():
    """calls of growing and shrinking size on two streams nothing has run on yet: every first call on a stream takes per-call blocks (the ``extra`` path of
    csrc/scratch.hip), every larger one regrows that stream's arena -- the sizes of tests/test_wsinterpd.py test_temporaries_of_interleaved_streams_do_not_collide"""
    from qups_amd.interpd import shift_sum
    rng = np.random.default_rng(7)
    calls = []
    for k, (M, Mo) in enumerate([(5, 3), (40, 33), (7, 2), (64, 64), (3, 70), (64, 64)]):
        T, N = 300 + 17 * k, 4
        x = _dev((rng.standard_normal((T, N, M)) + 1j * rng.standard_normal((T, N, M))).astype(np.complex64))
        sh, w = _dev(rng.uniform(-20, 20, (M, Mo)).astype(np.float32).astype(np.float64)), _dev(rng.uniform(0.2, 1, (M, Mo)))
        calls.append(lambda x=x, sh=sh, w=w: shift_sum(x, sh, w, "cubic"))
    ST.interleaved(calls, torch.cuda.Stream(), torch.cuda.Stream(), FILL_MS * len(calls))
    SEEN.setdefault("arena_regrow", [0, 0])[0] += 1


# ================================================================================================================ the two cache races
def test_shift_table_memo_checks_M_before_the_lookup(monkeypatch):
    """the same host table with data of another M: DasError, and qdas_shift_sum is not called (the memo's key holds the table's shape, not the data's M; a hit
    used to return in front of the check and the kernel read a wrong-sized table)"""
    from qups_amd import _lib
    from qups_amd.das_spec import DasError
    from qups_amd.interpd import shift_sum
    from tests import test_gpu_guards as TG
    x, shift, w, pad = TG._shift_case("complex64")
    L = _lib.lib()
    real, calls = L.qdas_shift_sum, []

    def recorder(*a):
        calls.append(a)
        return real(*a)
    monkeypatch.setattr(L, "qdas_shift_sum", recorder)
    y = shift_sum(_dev(x), shift, w, "cubic")                  # the table is in the memo now
    torch.cuda.synchronize()
    assert len(calls) == 1
    for M2 in (x.shape[2] + 2, x.shape[2] - 3):
        x2 = torch.zeros((x.shape[0], x.shape[1], M2), dtype=torch.complex64, device="cuda")
        with pytest.raises(DasError, match="shift_sum: shift must be M x Mo"):
            shift_sum(x2, shift, w, "cubic")
    assert len(calls) == 1, "qdas_shift_sum was called with a table that does not fit the data"
    del y


def test_an_evicted_shift_table_stays_valid_for_a_call_queued_on_another_stream(side):
    """table A is built on s1; ``shift_sum(x, A)`` is queued on s2 behind a filler (a memo hit: no wait); eight further tables of the SAME shape (every read stays in
    bounds) go through the memo on s1 and evict A, whose block belongs to s1's allocator pool; more tables of that shape are allocated on s1.  The s2
    result must be the serial one, bit for bit."""
    from qups_amd import interpd
    from qups_amd.interpd import shift_sum
    s1, s2 = side
    rng = np.random.default_rng(77)
    T, N, M, Mo = 300, 4, 64, 64
    x = _dev((rng.standard_normal((T, N, M)) + 1j * rng.standard_normal((T, N, M))).astype(np.complex64))
    tab = lambda: (rng.uniform(-20, 20, (M, Mo)).astype(np.float32).astype(np.float64), rng.uniform(0.2, 1, (M, Mo)))
    A = tab()
    others = [tab() for _ in range(8)]
    ref = shift_sum(x, *A, "cubic").clone()
    torch.cuda.synchronize()
    for s in (s1, s2):                                         # both streams' arenas (csrc/scratch.hip) at their size for this shape: a regrow frees blocks with hipFree,
        with torch.cuda.stream(s):                             # which waits for the whole device -- the filler included
            for _ in range(3):
                shift_sum(x, *tab(), "cubic")
    torch.cuda.synchronize()
    with interpd._SHIFT_MEMO_LOCK:
        interpd._SHIFT_MEMO.clear()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        shift_sum(x, *A, "cubic")                              # A's device copies: blocks of s1's pool
    torch.cuda.synchronize()
    ev = ST.filler(s2, 10 * FILL_MS)                           # (one FILL_MS per wrapper call issued while it runs: the hit, eight tables, the allocations)
    with torch.cuda.stream(s2):
        y = shift_sum(x, *A, "cubic")                          # queued behind the filler
    assert ST.returned_early(ev), "the memo hit waited: the race below was not set up"
    junk = []
    with torch.cuda.stream(s1):
        for sh, w in others:
            shift_sum(x, sh, w, "cubic")
        for _ in range(64):                                    # whatever block A's copies gave back is taken again, and overwritten, on s1
            junk.append(torch.full((Mo, M), float("nan"), dtype=torch.float32, device="cuda"))
    assert ST.returned_early(ev), "the filler ended before the tables were evicted: the race was not set up"
    torch.cuda.synchronize()
    assert same_bits(y, ref), "a table evicted from the memo was handed out again while a call queued on another stream still read it"


def test_hilbert_never_executes_a_destroyed_plan(monkeypatch):
    """``clear_pre_plan_cache()`` between ``_pre_plan`` and the execute (an eviction by another thread in that gap): no execute on a destroyed handle, and the
    result is right.  The library sees live handles only, before and after the fix: the stand-ins below record and drop calls on dead ones."""
    from qups_amd import _lib, preproc
    from tests.test_preproc import hilbert_ref
    L = _lib.lib()
    preproc.clear_pre_plan_cache()
    real_destroy, real_exec, real_one = L.qdas_pre_plan_destroy, L.qdas_pre_execute, L.qdas_pre_plan_one_pass
    dead, on_dead = set(), []
    val = lambda h: h.value if isinstance(h, C.c_void_p) else int(h)

    def destroy(h):
        dead.add(val(h))
        return real_destroy(h)

    def execute(h, *a):
        if val(h) in dead:
            on_dead.append(("qdas_pre_execute", val(h)))
            return 0
        return real_exec(h, *a)

    def one_pass(h):
        if val(h) in dead:
            on_dead.append(("qdas_pre_plan_one_pass", val(h)))
            return 0
        return real_one(h)
    monkeypatch.setattr(L, "qdas_pre_plan_destroy", destroy)
    monkeypatch.setattr(L, "qdas_pre_execute", execute)
    monkeypatch.setattr(L, "qdas_pre_plan_one_pass", one_pass)
    real_plan, n = preproc._pre_plan, [0]

    def pre_plan(key, d):
        e = real_plan(key, d)
        n[0] += 1
        if n[0] == 1:
            preproc.clear_pre_plan_cache()                     # "another thread" empties the cache while this call holds its entry
        return e
    monkeypatch.setattr(preproc, "_pre_plan", pre_plan)
    x = np.random.default_rng(12).standard_normal((300, 5)).astype(np.float32)
    y = preproc.hilbert(_dev(x), 512)
    torch.cuda.synchronize()
    assert n[0] >= 1 and not on_dead, f"hilbert used a destroyed plan: {on_dead}"
    ref = hilbert_ref(x.astype(np.float64), 512)
    assert np.abs(_np(y) - ref).max() / np.abs(ref).max() <= 2e-5          # (tests/test_preproc.py's bound)
    assert len(dead) == 1, "the plan that left the cache is destroyed by its last user"
    monkeypatch.undo()
    preproc.clear_pre_plan_cache()


# ================================================================================================================ the harness can fail
def test_the_harness_reports_a_step_on_the_wrong_stream(side):
    """torch-only stand-ins, no library code: an "entry" that computes under the default stream reads its delayed input early (poison), one that
    launches its last step on another stream is caught by the consumer, and one that synchronises is seen to block"""
    x = torch.randn(1 << 16, device="cuda")
    ref = x * 2 + 1
    torch.cuda.synchronize()

    def good(a):
        return a * 2 + 1

    def wrong_stream(a):
        with torch.cuda.stream(torch.cuda.default_stream()):
            return a * 2 + 1

    def blocking(a):
        y = a * 2 + 1
        torch.cuda.current_stream().synchronize()
        return y
    (o,), (c,), early = ST.run_delayed(good, [x], side[0], FILL_MS)
    assert same_bits(o, ref) and same_bits(c, ref) and early
    (o,), (c,), early = ST.run_delayed(wrong_stream, [x], side[0], FILL_MS)
    assert early
    assert not same_bits(o, ref) and bool(torch.isnan(o).all()), "the test no longer sees what it guards against"
    (o,), (c,), early = ST.run_delayed(blocking, [x], side[0], FILL_MS)
    assert same_bits(o, ref) and not early, "the test no longer sees what it guards against"
    # the same through the case table's own checks: a BLOCKS entry that returns early and an unlisted one that blocks both fail
    CASES["selftest-good"] = ("selftest", True, None, contextlib.contextmanager(lambda: (yield dict(fn=good, tensors=[x]))))
    CASES["selftest-wrong"] = ("selftest", True, None, contextlib.contextmanager(lambda: (yield dict(fn=wrong_stream, tensors=[x]))))
    CASES["selftest-blocking"] = ("selftest", True, None, contextlib.contextmanager(lambda: (yield dict(fn=blocking, tensors=[x]))))
    try:
        if not os.environ.get("QDAS_STREAMS_MEASURE"):
            _check_case("selftest-good", side[0])
            failed = []
            for cid, blocks in (("selftest-wrong", BLOCKS), ("selftest-blocking", BLOCKS), ("selftest-good", dict(BLOCKS, selftest="listed, but it does not wait"))):
                try:
                    _check_case(cid, side[0], blocks=blocks)
                except AssertionError:
                    failed.append(cid)
            assert failed == ["selftest-wrong", "selftest-blocking", "selftest-good"], f"the test no longer sees what it guards against: {failed}"
    finally:
        for cid in ("selftest-good", "selftest-wrong", "selftest-blocking"):
            CASES.pop(cid, None)
        SEEN.pop("selftest", None)


# ================================================================================================================ summary
def test_zz_every_entry_ran_on_a_side_stream(request, capsys):
    """one line per entry -- cases, whether it blocked -- so that an entry whose cases were all deselected shows"""
    want = {e for e, _, _, _ in CASES.values()}
    lines = [f"streams: {name:18s} cases={n:3d} blocked={b:3d} {'(BLOCKS: ' + BLOCKS[name].split(' -- ')[0] + ')' if name in BLOCKS else ''}" for name, (n, b) in SEEN.items()]
    lines += [f"streams: {name:18s} cases=  0 result=NOT RUN" for name in sorted(want - set(SEEN))]
    if HOST_MS:
        worst = max(HOST_MS, key=HOST_MS.get)
        lines.append(f"streams: largest host time of a warm call on the default stream: {HOST_MS[worst]:.2f} ms ({worst}); FILL_MS={FILL_MS}; {len(CASES)} table rows")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    ran_all = sum(1 for i in request.session.items if i.module.__name__ == __name__ and getattr(i, "originalname", "") == "test_delayed_producer_and_consumer") == len(CASES)
    if ran_all and not os.environ.get("PYTEST_XDIST_WORKER"):
        assert not (want - set(SEEN)), sorted(want - set(SEEN))
