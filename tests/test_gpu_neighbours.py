"""Loud neighbours and isolation between the members of every batched 1-D entry (helper: tests/neighbours.py, proved on the CPU by
tests/test_neighbours_host.py).

One table of rows.  Each names the smallest shape at which the members straddle the boundaries its kernel has, the axes that enumerate members, the wrapper call
and the float64 restatement of the entry's home test file (imported from there).  Checks: A = exact scale equivariance under per-member powers of two, B = parity
per member over that member's own ``max|ref|`` within the home file's bound, C = NaN / +Inf in every other member changes no bit of the rest.

The rows' inputs are built on the CPU, so tests/test_neighbours_host.py can check there, from the restatements alone, that every scaled run stays far inside the
normal range.  The last test prints ``entry -> cases, members`` per check and asserts that every row ran each check it is marked for."""
import functools
import importlib
import os

import numpy as np
import pytest
import torch

from tests import neighbours as NB

pytestmark = pytest.mark.gpu

FS, T0 = 20e6, 1.7e-6                                   # tests/test_preproc.py test_one_pass_hilbert_matches_numpy
HILBERT_BOUND = 2e-5                                    # tests/test_preproc.py test_hilbert_matches_numpy and test_one_pass_hilbert_matches_numpy: `<= 2e-5` of max|ref|
HALF_BOUND = 1.5e-3                                     # tests/test_convd.py test_convd_half_precision: `<= 1.5e-3 * np.abs(ref).max()`
WORST = {}                                              # B rows: entry -> largest per-unit error / bound seen

ROWS = []


class Row:
    def __init__(self, entry, name, prec, checks, make, in_axes, out_axes, call, ref, group=1, degree=1, same=False, env=None, after=None, bound=None):
        self.entry, self.name, self.prec, self.checks = entry, name, prec, checks
        self.make, self.in_axes, self.out_axes, self.call, self.ref = make, in_axes, out_axes, call, ref
        self.group, self.degree, self.same, self.env, self.after, self.bound = group, degree, same, env or {}, after, bound
        ROWS.append(self)

    def inputs(self):
        return [t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t)) for t in self.make()]

    def spec(self, guard=None):
        return NB.Spec(self.in_axes, self.out_axes, group=self.group, guard=guard, degree=self.degree, seed=len(self.name))


def _n(t):
    """a CPU tensor as the float64 / complex128 numpy values the device sees"""
    if t.dtype == torch.complex32:
        return torch.view_as_real(t).double().numpy().view(np.complex128)[..., 0]
    return t.numpy().astype(np.complex128 if t.is_complex() else np.float64)


def _randn(seed, shape, dtype):
    rng = np.random.default_rng(seed)
    if dtype == "i16":
        return np.clip(np.round(rng.standard_normal(shape) * 600), -2000, 2000).astype(np.int16)
    dt = np.dtype(dtype)
    v = rng.standard_normal(shape)
    if dt.kind == "c":
        v = v + 1j * rng.standard_normal(shape)
    return v.astype(dt)


def _half(a, cplx):
    """numpy float data -> a torch half / complex-half tensor"""
    if not cplx:
        return torch.from_numpy(a.astype(np.float16))
    return torch.view_as_complex(torch.from_numpy(np.stack([a.real, a.imag], -1).astype(np.float16)).contiguous())


# ================================================================================================================ hilbert
def _hilbert_row(entry, T, N, rest, dtype, fdown, one_pass, group, checks, env=None):
    from tests.test_preproc import hilbert_ref

    def call(x):
        from qups_amd.preproc import hilbert
        y = hilbert(x, N, fdown, T0, FS)
        assert hilbert.last_one_pass == one_pass, "the row did not take the path it names"
        return y

    def after(row, spec, inputs, clean, runs, monkeypatch):
        """``fdown = 0``: the real part IS the (zero-padded, truncated) input, bit for bit, for every trace of the clean run and under every poison pattern"""
        if fdown or not one_pass:
            return
        for ins, outs in [(inputs, clean)] + [(r[2], r[3]) for r in runs]:
            x = ins[0].float()
            want = torch.zeros((N,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
            want[:min(T, N)] = x[:min(T, N)]
            assert torch.equal(NB.bits(outs[0].real.contiguous()), NB.bits(want)), "the real part is not the input"

    axes = tuple(range(1, 1 + len(rest)))
    Row(entry, f"{entry} N={N} T={T} x{'x'.join(map(str, rest))} {dtype} fdown={fdown:g}", "f32", checks,
        lambda: [_randn(T + 7 * len(rest), (T,) + rest, "i16" if dtype == "i16" else np.float32)], [axes], axes, call,
        lambda x: hilbert_ref(_n(x), N, fdown, T0, FS), group=group, env=env, after=after, bound=HILBERT_BOUND)


for _dt in ("f32", "i16"):
    for _fd in (0.0, 3.3e6):
        for _rest in ((5,), (3, 3)):                                  # K = 5, and 3 channels x 3 transmits: pairs straddle transmits, the last trace is single
            _hilbert_row("hilbert fixed list", 256, 256, _rest, _dt, _fd, True, 2, "ABC")          # 256 = 16 16
        _hilbert_row("hilbert run-time list", 180, 210, (4,), _dt, _fd, True, 2, "ABC")             # 210 = 7 5 3 2, T = 180 zero-padded
for _N in (3072, 5632):                                               # 3 16 8 8 (fixed) and 11 8 8 8 (run-time): the 512-thread variant
    _hilbert_row("hilbert 512-thread lists", _N, _N, (3,), "f32", 0.0, True, 2, "ABC")
    _hilbert_row("hilbert 512-thread lists", _N, _N, (3,), "i16", 3.3e6, True, 2, "ABC")
for _dt in ("f32", "i16"):
    _hilbert_row("hilbert hipFFT passes", 301, 301, (5,), _dt, 0.0, False, 1, "AC")                 # 301 = 7 x 43: trace by trace
    _hilbert_row("hilbert hipFFT passes", 256, 256, (5,), _dt, 3.3e6 if _dt == "i16" else 0.0, False, 1, "AC", env={"QDAS_PRE_HIPFFT": "1"})


# ================================================================================================================ convd
def _convd_ref(dim, shape):
    from oracle import convd_oracle as O
    return lambda x, y: O.convd(_n(x), _n(y), dim, shape)[0]


def _convd_call(dim, shape):
    def call(x, y):
        from qups_amd import convd
        return convd(x, y, dim, shape)
    return call


def _direct_path_taken(row, spec, inputs, clean, runs, monkeypatch):
    """complex64 traces with ONE filter of >= 128 taps would go to the FFT convolution (csrc/conv.hip qdas_convd): the row switches it off, and here shows that it did --
    forced onto the FFT path the same call rounds differently (tests/test_convd.py test_convd_long_filters_take_the_fft_path)"""
    monkeypatch.setenv("QDAS_CONV_FFT_MIN_TAPS", "90")
    fft = row.call(*inputs)
    assert not torch.equal(NB.bits(fft), NB.bits(clean[0])), "the row ran the FFT path, not the direct kernel it names"


# time contiguous (the filtered dimension is the fastest in memory: the LDS kernel): 5 slices of 1100 samples -- two 1024-output tiles; 37 taps, 300 taps (two
# 256-tap chunks), one filter per slice.  QDAS_CONV_FFT_MIN_TAPS keeps every row on the direct kernel (the FFT path has rows of its own below)
for _dt, _prec in ((np.float32, "f32"), (np.complex64, "f32"), (np.complex128, "f64")):
    for _shape in ("full", "same"):
        for _ysz, _yax in (((1, 37), None), ((1, 300), None), ((5, 37), 0)):
            Row("convd time-contiguous", f"convd contiguous x(5,1100) y{_ysz} {_shape} {np.dtype(_dt).name}", _prec, "AC",
                functools.partial(lambda dt, ysz: [_randn(1, (5, 1100), dt), _randn(2, ysz, dt)], _dt, _ysz), [0, _yax], 0,
                _convd_call(2, _shape), _convd_ref(2, _shape), env={"QDAS_CONV_FFT_MIN_TAPS": "1000000", "QDAS_CONV_NO_FFT": None},
                after=_direct_path_taken if (_dt is np.complex64 and _ysz == (1, 300)) else None)
# strided: 70 columns (fast) x 3 slices, 40 samples, 9 taps: one filter per column, and one for all
for _ysz, _yax in (((1, 9, 70), (None, 2)), ((1, 9, 1), None)):
    Row("convd strided", f"convd strided x(3,40,70) y{_ysz}", "f32", "AC",
        functools.partial(lambda ysz: [_randn(3, (3, 40, 70), np.complex64), _randn(4, ysz, np.complex64)], _ysz), [(0, 2), _yax], (0, 2),
        _convd_call(2, "full"), _convd_ref(2, "full"))
# half and complex-half storage: B and C only (subnormal half outputs are not scale-exact)
for _cplx in (False, True):
    Row("convd half", f"convd half x(3,1100) y(1,37) {'complex' if _cplx else 'real'}", "f16", "BC",
        functools.partial(lambda cplx: [_half(0.25 * _randn(5, (3, 1100), np.complex64 if cplx else np.float32), cplx),
                                        _half(0.25 * _randn(6, (1, 37), np.complex64 if cplx else np.float32), cplx)], _cplx), [0, None], 0,
        _convd_call(2, "same"), _convd_ref(2, "same"), bound=HALF_BOUND)


# the FFT path: complex64 traces, time contiguous, one filter of 129 taps
def _fft_path_taken(row, spec, inputs, clean, runs, monkeypatch):
    """as tests/test_convd.py test_convd_long_filters_take_the_fft_path: the two paths round differently -- identical bits mean the FFT path did not run"""
    monkeypatch.setenv("QDAS_CONV_FFT_MIN_TAPS", "1000000")
    direct = row.call(*inputs)
    assert not torch.equal(NB.bits(direct), NB.bits(clean[0])), "the FFT path did not run"


for _ct in (False, True):
    Row("convd FFT path", f"convd fft x(5,700) 129 {'complex' if _ct else 'real'} taps", "f32", "AC",
        functools.partial(lambda ct: [_randn(7, (5, 700), np.complex64), _randn(8, (1, 129), np.complex64 if ct else np.float32) * np.hanning(129).astype(np.float32)], _ct),
        [0, None], 0, _convd_call(2, "full"), _convd_ref(2, "full"), env={"QDAS_CONV_FFT_MIN_TAPS": "90", "QDAS_CONV_NO_FFT": None}, after=_fft_path_taken)


# ================================================================================================================ sosfilt
@functools.lru_cache(maxsize=None)
def _sos():
    from scipy import signal
    return signal.butter(4, [0.1, 0.4], "band", output="sos")[:2]          # two sections


def _sos_call(x):
    from qups_amd import sosfilt
    return sosfilt(x, _sos(), 1, 0.5)


def _sos_ref(x):
    from oracle import convd_oracle as O
    return O.sosfilt(_n(x), _sos(), 0, 0.5)


# T = 45 (a 32-sample tile and 13), K = 67 traces (64 per workgroup and 3; an odd count: the last wave-wide load of two real traces holds one)
for _dt, _prec in ((np.float32, "f32"), (np.complex64, "f32"), (np.complex128, "f64")):
    Row("sosfilt", f"sosfilt x(45,67) {np.dtype(_dt).name}", _prec, "AC", functools.partial(lambda dt: [_randn(9, (45, 67), dt)], _dt), [1], 1, _sos_call, _sos_ref)


# ================================================================================================================ shift_sum
@functools.lru_cache(maxsize=None)
def _shift_w():
    rng = np.random.default_rng(31)
    shift = rng.uniform(-20, 20, (6, 4)).astype(np.float32).astype(np.float64)
    shift[0, 0], shift[1, 1], shift[2, 2] = -200.0, 200.0, 2.5             # nothing in range twice; a half-integer
    w = rng.uniform(0.2, 1, (6, 4))
    w[rng.random((6, 4)) < 0.2] = 0
    return shift, w


def _unforced_shift_sum_passes_taps_between_lanes(To, taps):
    """csrc/shiftsum.hip launch_shift_sum restated for complex64 with no switch set: the outputs per lane ``best`` among 4 / 3 / 2, and the lane-passing variant only
    where ``best == 3`` and its groups of ``65 - taps`` outputs need no more blocks per trace.  (The library has no query for the variant that ran.)"""
    best, waste = 4, None
    for tpt in (4, 3, 2):
        cov = -(-To // (256 * tpt)) * 256 * tpt - To
        if waste is None or (cov < waste and (waste - cov) * 16 > To):
            best, waste = tpt, cov
    tpd = 12 * (65 - taps)
    return taps > 1 and best == 3 and -(-To // tpd) <= -(-To // 768)


def _shift_row(interp, dt, prec, dpp):
    def call(x):
        from qups_amd.interpd import shift_sum
        shift, w = _shift_w()
        # QDAS_SS_DPP is read as "set or not" (csrc/shiftsum.hip: getenv(..) != nullptr): the rows without ``dpp`` leave it ABSENT, as tests/test_wsinterpd.py does,
        # and at To = 96 the planner then takes 2 outputs per lane: the ordinary kernel
        assert ("QDAS_SS_DPP" in os.environ) == dpp and "QDAS_SS_NO_DPP" not in os.environ and "QDAS_SS_TPT" not in os.environ
        assert dpp or not _unforced_shift_sum_passes_taps_between_lanes(x.shape[0], {"linear": 2, "cubic": 4, "lanczos3": 6}[interp])
        return shift_sum(x, shift, w, interp)

    def ref(x):
        from tests.test_wsinterpd import _shift_ref
        shift, w = _shift_w()
        return _shift_ref(_n(x), shift, w, interp, x.shape[0])
    # x is T x N x M x F: the M transmits are summed; receive channels n and frames f are the members
    Row("shift_sum", f"shift_sum x(96,5,6,2) {interp} {np.dtype(dt).name}{' dpp' if dpp else ''}", prec, "AC",
        functools.partial(lambda: [_randn(10, (96, 5, 6, 2), dt)]), [(1, 3)], (1, 3), call, ref,
        env={"QDAS_SS_DPP": "1" if dpp else None, "QDAS_SS_NO_DPP": None, "QDAS_SS_TPT": None})


for _interp in ("linear", "cubic", "lanczos3"):
    _shift_row(_interp, np.complex64, "f32", False)
    _shift_row(_interp, np.complex64, "f32", True)                          # lane-to-lane taps (tests/test_wsinterpd.py's ``dpp``): complex64 only
    _shift_row(_interp, np.float32, "f32", False)
    _shift_row(_interp, np.complex128, "f64", False)


# ================================================================================================================ pwznxcorr
def _pw_row(ref_kind, dt, norm):
    kw = dict(zero=True, norm=norm, ref=ref_kind)

    def call(x):
        from qups_amd import pwznxcorr
        return pwznxcorr(x, 3, 8, **kw)

    def ref(x):
        from tests import pwznxcorr_ref as R
        return R.pwznxcorr(_n(x), 3, 8, **kw)
    # x is T x N x 5: every output correlates two channels of ONE page, so it is of degree 2 in the page (norm=False) or of degree 0 (norm=True)
    Row("pwznxcorr", f"pwznxcorr x(80,6,5) {ref_kind} {np.dtype(dt).name} norm={norm}", "f32", "AC",
        functools.partial(lambda: [_randn(11, (80, 6, 5), dt)]), [2], 2, call, ref, degree=2, same=norm)


for _rk in ("neighbor", "center"):
    for _dt in (np.complex64, np.float32):
        for _norm in (False, True):
            _pw_row(_rk, _dt, _norm)


# ================================================================================================================ refocus
@functools.lru_cache(maxsize=None)
def _decoder(T):
    """tikhonov decoding pages of a focused sequence (tests/refocus_ref.py), M = 6 elements x V = 4 pulses, as complex64 values"""
    from tests import refocus_ref as R
    tau, _, _ = R.fc_sequence(6, 4)
    return R.decoder(tau, np.ones((6, 4)), T, FS, "tikhonov", None, 17).astype(np.complex64).astype(np.complex128)


def _refocus_row(T, layout, kind):
    t0 = 1.3e-6 if kind == "scalar" else 1.3e-6 + (np.arange(4)[::-1] * 0.37 + 0.21) / FS          # tests/test_gpu_refocus.py _t0

    def call(x):
        from qups_amd import refocus as RF
        assert RF.takes(T)
        return RF.fused(x, t0, FS, RF.Decoder(_decoder(T)))

    def ref(x):
        from tests import refocus_ref as R
        return R.apply(_n(x), t0, FS, _decoder(T))[0]
    # x is T x N x V x frames: the V pulses are decoded into M elements; receive channels n and frames are the members (C = 34 traces of 16 per workgroup)
    Row("refocus", f"refocus T={T} ({layout}) N=17 V=4 M=6 frames=2 t0={kind}", "f32", "AC",
        functools.partial(lambda: [_randn(12 + T, (T, 17, 4, 2), np.complex64)]), [(1, 3)], (1, 3), call, ref)


# the three workgroup layouts of csrc/refocus.hip qdas_refocus (``nth`` threads per trace from fft_factor, ``ngrp = 2`` where ``2 nth <= 512``):
#   T = 64   = 8 8:        nth = 64, two thread groups per workgroup, a trace each
#   T = 1050 = 7 5 5 3 2:  the 512-thread variant's stage list with 263 butterflies -> nth = 320: ONE group
#   T = 770  = 11 7 5 2:   the 512-thread variant, nth = 256: two groups of 256 threads
for _T, _layout in ((64, "two groups"), (1050, "one group"), (770, "512 threads")):
    for _kind in ("scalar", "per-pulse"):
        _refocus_row(_T, _layout, _kind)


# ================================================================================================================ migration
def _mig_row(keep_tx):
    def make():
        from tests import test_gpu_migration as H
        T, N, M, _ = H.SHAPES[0]
        return [H._data(T, N, M, 3)[0]]

    def call(x):
        from qups_amd import migration as MG
        from tests import test_gpu_migration as H
        T, N, M, nfft = H.SHAPES[0]
        _, tau, gam = H._data(T, N, M, 3)
        return MG.migrate(x, H.T0, H.FS, tau, gam, H.PITCH, H.C0, nfft, 0.0, "cubic", True, keep_tx)

    def ref(x):
        from tests import migration_ref as R
        from tests import test_gpu_migration as H
        T, N, M, nfft = H.SHAPES[0]
        _, tau, gam = H._data(T, N, M, 3)
        return R.migrate(_n(x), H.T0, H.FS, tau, gam, H.PITCH, H.C0, nfft, 0.0, "cubic", True, keep_tx)
    # x is T x N x M x frames; the transform runs over T and N.  Summed: frames are the members; keep_tx: transmits and frames
    Row("migrate", f"migrate 64x16x3 frames=3 keep_tx={keep_tx}", "f32", "AC", make, [(2, 3) if keep_tx else 3], (2, 3) if keep_tx else 2, call, ref)


_mig_row(False)
_mig_row(True)


# ================================================================================================================ scan_convert
def _sc_row(name, P, dt, pre):
    three = name.count("x") == 2
    nd = 3 if three else 2

    def case():
        from tests import scanconvert_ref as R
        return R.spherical_case(name) if three else R.polar_case(name)

    def make():
        from tests import scanconvert_ref as R
        c = case()
        return [R.data(tuple(c[k].size for k in (("r", "a", "e") if three else ("r", "a"))) + (P,), dt, 11)]

    def call(b):
        from qups_amd import scanconvert as SC
        c = case()
        if three:
            return SC.scan_convert3(b, *(np.array(c[k]) for k in ("r", "a_deg", "e_deg")), c["origin"], *(np.array(c[k]) for k in ("x", "y", "z")), pre=pre)[0]
        return SC.scan_convert(b, np.array(c["r"]), np.array(c["a_deg"]), c["origin"], np.array(c["x"]), np.array(c["z"]), pre=pre)[0]

    def ref(b):
        from tests import scanconvert_ref as R
        c = case()
        if three:
            return R.convert_spherical(_n(b), c["r"], c["a"], c["e"], c["origin"], c["x"], c["y"], c["z"], pre=pre)[0]
        return R.convert_polar(_n(b), c["r"], c["a"], c["origin"], c["x"], c["z"], pre=pre)[0]
    Row("scan_convert3" if three else "scan_convert", f"scan_convert {name} P={P} {np.dtype(dt).name} pre={pre}", "f32", "AC", make, [nd], nd, call, ref)


for _dt in (np.float32, np.complex64):
    for _pre in ("none", "abs"):
        _sc_row("2x2", 3, _dt, _pre)
        _sc_row("2x2x2", 2, _dt, _pre)


# ================================================================================================================ ray_integrals, ray_backproject
def _ray_rows(dtype, ord):
    name = "2x2"
    nt = np.float32 if dtype == torch.float32 else np.float64

    def case():
        from tests import test_gpu_raybackproject as H
        return H.case(name, dtype)

    def maps():
        c = case()
        shape = (3, c["Z"], c["X"]) if ord == "ZX" else (3, c["X"], c["Z"])
        return [_randn(13, shape, nt)]

    def integ(m):
        from qups_amd import raypaths as RP
        c = case()
        return RP.ray_integrals(m, c["xg"], c["zg"], c["pa"], c["pb"], ord=ord)[0]

    def integ_ref(m):
        mm = _n(m)
        return np.einsum("jxz,fxz->fj", case()["W"], mm if ord == "XZ" else mm.transpose(0, 2, 1))

    def back(r):
        from qups_amd import raypaths as RP
        c = case()
        return RP.ray_backproject(r, c["xg"], c["zg"], c["pa"], c["pb"], ord=ord)

    def back_ref(r):
        g = np.einsum("jxz,fj->fxz", case()["W"], _n(r))
        return g if ord == "XZ" else g.transpose(0, 2, 1)
    prec = "f32" if dtype == torch.float32 else "f64"
    Row("ray_integrals", f"ray_integrals {name} F=3 {ord} {prec}", prec, "AC", maps, [0], 0, integ, integ_ref)
    Row("ray_backproject", f"ray_backproject {name} F=3 {ord} {prec}", prec, "AC", lambda: [np.array(case()["r"]).astype(nt)], [0], 0, back, back_ref)


for _dtype in (torch.float32, torch.float64):
    for _ord in ("ZX", "XZ"):
        _ray_rows(_dtype, _ord)


# ================================================================================================================ demod, resample, filtfilt: A only (their home files hold C)
def _demod_rows(dtname):
    K, ratio, p, q = 25, 4, 3, 2

    def x():
        return [_randn(14, (300, 5), "i16" if dtname == "i16" else np.float32)]

    def demod(x):
        from qups_amd.demod import demod as py_demod
        from tests import test_gpu_demod as H
        return py_demod(x, H.FC, H.FS, H.T0, H.taps(K), ratio)

    def demod_ref(x):
        from tests import demod_ref as R
        from tests import test_gpu_demod as H
        return R.demod(_n(x), H.FC, H.FS, H.T0, H.taps(K), ratio)

    def resample(x):
        RS = importlib.import_module("qups_amd.resample")               # (the package exports the function under the module's name)
        return RS.resample(x, p, q)

    def resample_ref(x):
        from scipy.signal import resample_poly
        RS = importlib.import_module("qups_amd.resample")               # (the package exports the function under the module's name)
        return resample_poly(_n(x), p, q, axis=0, window=RS.resample_taps(p, q) / p)

    def filtfilt(x):
        RS = importlib.import_module("qups_amd.resample")               # (the package exports the function under the module's name)
        from tests import test_gpu_demod as H
        return RS.filtfilt(H.taps(K + 1), x)

    def filtfilt_ref(x):
        from scipy.signal import filtfilt as ff
        from tests import test_gpu_demod as H
        return np.ascontiguousarray(ff(H.taps(K + 1), [1.0], _n(x), axis=0, padlen=3 * K))
    Row("demod", f"demod x(300,5) {dtname}", "f32", "A", x, [1], 1, demod, demod_ref)
    Row("resample", f"resample 3/2 x(300,5) {dtname}", "f32", "A", x, [1], 1, resample, resample_ref)
    Row("filtfilt", f"filtfilt 26 taps x(300,5) {dtname}", "f32", "A", x, [1], 1, filtfilt, filtfilt_ref)


_demod_rows("i16")
_demod_rows("f32")


# ================================================================================================================ the test
@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.name)
def test_row(row, monkeypatch):
    for k, v in row.env.items():                                       # (None: the variable must be ABSENT -- some switches are read as "set or not")
        monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, v)
    spec = row.spec(guard=(monkeypatch, False))
    inputs = [t.cuda() for t in row.inputs()]
    clean = got = None
    if "A" in row.checks:
        clean, got = spec.check_scale(row.call, inputs, row.entry, row.name, same=row.same)
    if "B" in row.checks:
        xs, _ = spec.scaled(inputs)
        got = spec.run(row.call, xs) if got is None else got
        worst = spec.check_parity(got, row.ref(*[t.cpu() for t in xs]), row.bound, row.entry, row.name)
        WORST[row.entry] = max(WORST.get(row.entry, 0.0), worst / row.bound)
        print(f"neighbours B: {row.name}: largest per-unit error / own max|ref| = {worst:.3e} ({worst / row.bound:.3f} of the bound {row.bound:g})")
    runs = []
    if "C" in row.checks:
        runs = spec.check_poison(row.call, inputs, row.entry, row.name, clean=clean)
    if row.after is not None:
        row.after(row, spec, inputs, clean if clean is not None else spec.run(row.call, inputs), runs, monkeypatch)


def test_one_pass_hilbert_couples_the_two_traces_of_a_pair(monkeypatch):
    """the contract of ``hilbert``'s docstring from its other side: checked TRACE BY TRACE (``group=1``) the one-pass kernel fails A and C -- traces 2j and 2j+1 share a
    transform, so a trace's rounding follows its partner's exponent and a NaN reaches its partner's imaginary part (csrc/pre.hip HilbertOps::store:
    ``H x1 = Im - x2``, ``H x2 = x1 - Re``).  The rows above show that nothing crosses a PAIR.  Should the kernel ever equalise the exponents of a pair,
    A still fails here and C still must: this test then states which half of the contract moved."""
    from qups_amd.preproc import hilbert
    x = torch.from_numpy(_randn(3, (256, 5), np.float32)).cuda()
    spec = NB.Spec([1], 1, guard=(monkeypatch, False))
    call = lambda v: hilbert(v, 256)
    with pytest.raises(NB.NeighbourError, match="power of two"):
        spec.check_scale(call, [x])
    assert hilbert.last_one_pass
    with pytest.raises(NB.NeighbourError, match="unpoisoned units changed"):
        spec.check_poison(call, [x])
    xs, _ = spec.scaled([x])                                             # partners louder by 2^20 / 2^40: the quiet trace's error against its OWN maximum
    from tests.test_preproc import hilbert_ref
    with pytest.raises(NB.NeighbourError, match=r"max\|ref\|"):
        spec.check_parity(call(xs[0]), hilbert_ref(_n(xs[0].cpu())), HILBERT_BOUND)


def test_zz_every_row_ran_each_of_its_checks(request, capsys):
    """one line per entry -- cases and members per check -- so that an entry whose rows were all skipped shows"""
    want = {}
    for r in ROWS:
        want.setdefault(r.entry, set()).update(r.checks)
    lines = []
    for e, checks in want.items():
        seen = NB.SUMMARY.get(e, {})
        cells = " ".join(f"{c}: cases={seen.get(c, [0, 0])[0]:3d} members={seen.get(c, [0, 0])[1]:5d}" if c in checks else f"{c}: {'-':>23s}" for c in "ABC")
        worst = f" worst B = {WORST[e]:.3f} of its bound" if e in WORST else ""
        lines.append(f"neighbours: {e:26s} {cells}{worst} result={'ok' if all(seen.get(c, [0])[0] for c in checks) else 'NOT RUN'}")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    ran_all = sum(1 for i in request.session.items if i.module.__name__ == __name__ and getattr(i, "originalname", None) == "test_row") == len(ROWS)
    if ran_all and not os.environ.get("PYTEST_XDIST_WORKER"):          # (a selection with -k, or xdist workers, ran only part of the table)
        missing = [(e, c) for e, checks in want.items() for c in checks if not NB.SUMMARY.get(e, {}).get(c, [0])[0]]
        assert not missing, missing
