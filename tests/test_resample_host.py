"""qdas_resample without a GPU: the restatement tests/resample_ref.py against scipy (``upfirdn``, ``resample_poly``, ``filtfilt``), the default taps against
their closed form and ``firls x kaiser``, the design's own ripple on a tone, the time-axis rules of ``ChannelData.resample`` / ``filtfilt`` / ``fftfilt``, the
rational choice, the descriptor against the header, the C entry's validation (``device = -1``: nothing reaches a HIP call), the odd edge's reach rule, and the
kernel's index arithmetic (``csrc/resample_core.h``) walked on the CPU by a stand-alone program under AddressSanitizer and UBSan
(tests/resample_core_host.cpp) against the restatement.

The program evaluates in the kernel's order and precision (one accumulator, taps of a phase in ascending order, FMAs), so its error is the error of the
intended evaluation; every case must stay below the GPU test's bound ``(M + 4) eps S X`` (tests/resample_ref.py ``bound``)."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from qups_amd import _lib
from tests import resample_ref as R
from tests.test_streams_host import stream_entries

RS = importlib.import_module("qups_amd.resample")            # (the package exports the function under the module's name)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _x(T, Cn, cplx=False, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, Cn))
    return x + 1j * rng.standard_normal((T, Cn)) if cplx else x


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1e-300), np.abs(a - b).max() / np.abs(b).max()


# ---------------------------------------------------------------------------------------------------------------- the restatement against scipy
RATES = [(3, 2), (2, 3), (5, 4), (1, 4), (4, 1), (16, 25)]


@pytest.mark.parametrize("p,q", RATES)
def test_restatement_against_scipy_upfirdn_and_resample_poly(p, q):
    from scipy.signal import resample_poly, upfirdn
    x = _x(57, 2, True)
    h = np.random.default_rng(p + q).standard_normal(23)
    _close(R.upfirdn(h, x, p, q), upfirdn(h, x, p, q, axis=0))
    taps = RS.resample_taps(p, q, 3)
    _close(R.resample(x, p, q, taps), resample_poly(x, p, q, axis=0, window=taps / p))
    _close(R.resample(x.real, p, q, taps), resample_poly(x.real, p, q, axis=0, window=taps / p))


@pytest.mark.parametrize("K,T", [(2, 4), (9, 25), (26, 76), (5, 400), (129, 385)])
def test_restatement_against_scipy_filtfilt(K, T):
    from scipy.signal import filtfilt
    x = _x(T, 2, True, seed=K)
    b = np.random.default_rng(K).standard_normal(K)
    _close(R.filtfilt(b, x), filtfilt(b, [1.0], x, axis=0, padlen=3 * (K - 1)))


@pytest.mark.parametrize("p,q,K,off,edge", [(1, 1, 7, 3, "odd"), (3, 2, 11, 4, "zero"), (2, 3, 5, 0, "odd"), (16, 25, 40, 7, "zero"), (7, 4, 3, 2, "zero"), (6, 4, 9, 1, "odd")])
def test_the_vectorised_restatement_is_the_restatement(p, q, K, off, edge):
    x = _x(31, 2, True, seed=K)
    h = np.random.default_rng(K).standard_normal(K)
    J = (2 * 30 * p - off) // q if edge == "odd" else R.upfirdn_len(31, K, p, q) + 3
    _close(R.polyphase_fast(h, x, p, q, off, J, edge), R.polyphase(h, x, p, q, off, J, edge), 1e-14)


def test_filtfilt_with_one_tap_is_the_square():
    x = _x(7, 2, True)
    _close(R.filtfilt([0.75], x), 0.75 ** 2 * x)


# ---------------------------------------------------------------------------------------------------------------- the default taps
@pytest.mark.parametrize("p,q,n,beta", [(3, 2, 10, 5.0), (2, 3, 10, 5.0), (5, 4, 10, 5.0), (16, 25, 10, 5.0), (1, 32, 10, 5.0), (4, 1, 4, 8.0)])
def test_resample_taps(p, q, n, beta):
    from scipy.signal import firls
    h = RS.resample_taps(p, q, n, beta)
    pq = max(p, q)
    L = 2 * n * pq + 1
    assert h.shape == (L,) and h.dtype == np.float64
    assert np.abs(h - h[::-1]).max() <= 1e-16 * p and abs(h.sum() - p) <= 1e-13 * p
    assert np.abs(h - R.taps_closed_form(p, q, n, beta)).max() <= 1e-15 * p
    fc = 1.0 / (2 * pq)
    g = firls(L, [0, 2 * fc, 2 * fc, 1], [1, 1, 0, 0]) * np.kaiser(L, beta)
    assert np.abs(h - p * g / g.sum()).max() <= 1e-12 * p, "MATLAB's documented design: firls with a zero-width transition band, times the Kaiser window"


def test_resample_taps_reduces_and_refuses():
    assert np.array_equal(RS.resample_taps(6, 4), RS.resample_taps(3, 2))
    assert RS.resample_taps(1, 32).size == 641
    for bad in ((2, 2), (0, 1), (1.5, 2), (3, 2, 0)):
        with pytest.raises(RS.DasError):
            RS.resample_taps(*bad)


def test_a_tone_resampled_five_fourths():
    """cos(2 pi 0.05 t), 400 samples -> 500: outputs 100 .. 399 sit at times j 4/5.  The float64 restatement's own error is the design's ripple (1.63e-3); any
    correct evaluation in float32 arithmetic stays within twice that -- checked here on the stand-in for the device, float32 taps and data through the
    restatement, and in tests/test_gpu_resample.py on the device itself."""
    t = np.arange(400.0)
    x = np.cos(2 * np.pi * 0.05 * t)[:, None]
    h = RS.resample_taps(5, 4)
    y = R.resample(x, 5, 4, h)[:, 0]
    j = np.arange(100, 400)
    want = np.cos(2 * np.pi * 0.05 * j * 4 / 5)
    ripple = np.abs(y[j] - want).max()
    print(f"resample tone: the float64 restatement is within {ripple:.3e} of the tone")
    assert 1e-4 < ripple < 3e-3
    y32 = R.resample(x.astype(np.float32), 5, 4, h.astype(np.float32))[:, 0]
    assert np.abs(y32[j] - want).max() <= 2 * ripple


# ---------------------------------------------------------------------------------------------------------------- lengths, ABI
def test_lengths():
    L = _lib.lib()
    for T, p, q in ((0, 3, 2), (1, 1, 1), (7, 3, 2), (7, 2, 3), (2816, 5, 4), (2048, 16, 25), ((1 << 40) + 1, 4096, 4095), (5, 3, 0)):
        want = -(-T * p // q) if q else 0
        assert L.qdas_resample_len(T, p, q) == want
        if q:
            assert RS.resample_len(T, p, q) == want
    for T, K, p, q in ((1, 1, 1, 1), (7, 5, 3, 2), (57, 23, 16, 25), (0, 5, 3, 2), (7, 5, 3, 0)):
        want = -(-((T - 1) * p + K) // q) if q and T else 0
        assert L.qdas_upfirdn_len(T, K, p, q) == want
        if q:
            assert RS.upfirdn_len(T, K, p, q) == want


def test_abi_symbols_and_descriptor_layout():
    L = _lib.lib()
    for s in ("qdas_resample", "qdas_resample_len", "qdas_upfirdn_len"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
    D = _lib.ResampleDesc
    assert C.sizeof(D) == 9 * 8 + 4 * 4 + 8
    assert (D.J.offset, D.p.offset, D.off.offset, D.x_ld.offset, D.in_type.offset, D.edge.offset, D.device.offset, D.queue.offset) == (24, 32, 48, 56, 72, 76, 80, 88)
    with open(os.path.join(ROOT, "include", "qdas.h")) as f:
        header = f.read()
    body = re.search(r"typedef struct qdas_resample_desc \{(.*?)\} qdas_resample_desc;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            rest = decl.split(None, 1)[-1]
            names += [n.strip(" *") for n in rest.split(",")]
    assert names == [n for n, _ in D._fields_]
    codes = tuple(int(re.search(rf"#define QDAS_RESAMPLE_{n}\s+(\d+)", header).group(1)) for n in ("I16", "F32", "C64", "F64", "C128", "ZERO", "ODD", "MAX_K", "MAX_PQ"))
    assert codes == (_lib.RESAMPLE_I16, _lib.RESAMPLE_F32, _lib.RESAMPLE_C64, _lib.RESAMPLE_F64, _lib.RESAMPLE_C128, _lib.RESAMPLE_ZERO, _lib.RESAMPLE_ODD,
                     _lib.RESAMPLE_MAX_K, _lib.RESAMPLE_MAX_PQ)
    import qups_amd
    for n in ("resample", "resample_taps", "upfirdn", "filtfilt"):
        assert n in qups_amd.__all__ and callable(getattr(qups_amd, n))


BUF = (C.c_double * 8)()
P = C.cast(BUF, C.c_void_p)


def _desc(**kw):
    d = _lib.ResampleDesc()
    d.T, d.C, d.K, d.J, d.p, d.q, d.off, d.x_ld, d.out_ld = 100, 2, 5, 150, 3, 2, 2, 100, 150
    d.in_type, d.edge, d.device = _lib.RESAMPLE_F32, _lib.RESAMPLE_ZERO, -1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("kw,code,text", [
    (dict(p=0), 1, "p and q"), (dict(q=0), 1, "p and q"), (dict(K=0), 1, "at least one tap"), (dict(x_ld=99), 1, "x_ld"), (dict(out_ld=149), 1, "out_ld"),
    (dict(in_type=5), 1, "in_type"), (dict(in_type=-1), 1, "in_type"), (dict(edge=2), 1, "edge"), (dict(edge=-1), 1, "edge"),
    (dict(T=0, x_ld=0), 1, "T = 0"),
    (dict(K=_lib.RESAMPLE_MAX_K + 1), 2, "taps"), (dict(p=_lib.RESAMPLE_MAX_PQ + 1), 2, "rate"), (dict(q=_lib.RESAMPLE_MAX_PQ + 1), 2, "rate"),
    (dict(T=1 << 40, x_ld=1 << 40), 2, "2\\^40"), (dict(J=1 << 40, out_ld=1 << 40), 2, "2\\^40"), (dict(off=1 << 40), 2, "2\\^40"),
    (dict(C=1 << 31), 2, "workgroups"), (dict(J=1 << 39, out_ld=1 << 39, C=4), 2, "workgroups"),
    (dict(K=4096, p=1, q=1, in_type=_lib.RESAMPLE_C128), 2, "LDS"), (dict(K=8192, p=1, q=1, in_type=_lib.RESAMPLE_C64), 2, "LDS"),
    (dict(edge=1, p=1, q=1, off=0, J=100, out_ld=100, K=101), 1, "reach"), (dict(edge=1, p=1, q=1, off=0, J=300, out_ld=300, K=1), 1, "reach"),
])
def test_c_abi_rejects_bad_calls_before_any_launch(kw, code, text):
    """device = -1 and pointers to host memory: nothing here may reach a HIP call"""
    L = _lib.lib()
    assert L.qdas_resample(C.byref(_desc(**kw)), P, P, P) == code
    assert re.search(text, L.qdas_last_error().decode()), L.qdas_last_error()


def test_c_abi_null_pointers_and_empty_problems():
    L = _lib.lib()
    assert L.qdas_resample(None, P, P, P) == 1 and "null descriptor" in L.qdas_last_error().decode()
    for args, what in (((None, P, P), "x"), ((P, None, P), "h"), ((P, P, None), "out")):
        assert L.qdas_resample(C.byref(_desc()), *args) == 1 and f"null pointer ({what})" in L.qdas_last_error().decode()
    for kw in (dict(J=0), dict(C=0), dict(J=0, C=0, out_ld=0), dict(J=0, T=0, x_ld=0)):
        assert L.qdas_resample(C.byref(_desc(**kw)), None, None, None) == 0            # nothing to do, no device needed
    assert L.qdas_resample(C.byref(_desc(J=0, p=0)), None, None, None) == 1, "an empty call is still validated"
    # the limits themselves, and the extremes the entry promises to take, pass validation (the null pointer is reported first; the LDS budget is asked below)
    assert L.qdas_resample(C.byref(_desc(K=_lib.RESAMPLE_MAX_K, p=_lib.RESAMPLE_MAX_PQ, q=_lib.RESAMPLE_MAX_PQ)), None, P, P) == 1
    assert "null pointer" in L.qdas_last_error().decode()


def _geom(exe, K, p, q, eb, rb):
    r = subprocess.run([exe, "geom", str(K), str(p), str(q), str(eb), str(rb)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return dict(zip(("TJ", "lanes", "S", "Mmax", "rem", "span", "tap_bytes", "lds"), (int(v) for v in r.stdout.split())))


def test_the_lds_budget_takes_the_promised_extremes(core_exe):
    """every default design with max(p, q) <= 32 and filtfilt kernels up to 1025 taps, in all five types"""
    for eb, rb in ((4, 4), (8, 4), (8, 8), (16, 8)):
        for p, q in [(1, 32), (32, 1), (31, 32), (32, 31), (16, 25), (25, 16), (5, 4), (3, 32)]:
            g = _geom(core_exe, 2 * 10 * max(p, q) + 1, p, q, eb, rb)
            assert g["TJ"] >= 64 and g["lds"] <= 65536, (p, q, eb, g)
        g = _geom(core_exe, 1025, 1, 1, eb, rb)
        assert g["TJ"] >= 256 and g["lds"] <= 65536
    g = _geom(core_exe, 641, 1, 32, 16, 8)
    assert g["TJ"] == 64 and g["span"] == 63 * 32 + 641 and g["lds"] == g["tap_bytes"] + 16 * g["span"] <= 49 * 1024, "the issue's arithmetic: 43 KiB of span, 5 KiB of taps"
    assert _geom(core_exe, 641, 7, 4096, 4, 4)["TJ"] == 16 and _geom(core_exe, 641, 7, 4096, 16, 8)["TJ"] == 4      # fewer outputs when q / p is large
    assert _geom(core_exe, 4096, 1, 1, 16, 8)["TJ"] == 0 and _geom(core_exe, 2730, 1, 1, 16, 8)["TJ"] == 2 and _geom(core_exe, 8192, 1, 1, 4, 4)["TJ"] == 1
    assert _geom(core_exe, 8192, 2, 1, 16, 8)["TJ"] == 0 and _geom(core_exe, 8192, 2, 1, 4, 4)["TJ"] == 64 and _geom(core_exe, 4097, 4096, 7, 16, 8)["TJ"] == 1024
    for K, p, q, eb, rb in ((101, 5, 4, 4, 4), (1, 1, 1, 4, 4), (641, 4096, 7, 16, 8), (2048, 2047, 1, 16, 8)):
        g = _geom(core_exe, K, p, q, eb, rb)
        assert g["S"] == min(p, K) and g["Mmax"] == (K - 1) // p and g["rem"] == (K - 1) % p
        assert g["tap_bytes"] % 16 == 0 and 0 <= g["tap_bytes"] - K * rb < 16 and g["lanes"] == min(max(g["TJ"], 64), 256)
        assert g["span"] == -(-(g["TJ"] - 1) * q // p) + g["Mmax"] + 1


@pytest.mark.parametrize("off,J,p,q,K", [(0, 10, 1, 1, 5), (4, 10, 1, 1, 5), (7, 20, 3, 2, 11), (0, 9, 7, 4096, 3), (5, 40, 16, 25, 2), (0, 3, 8, 8, 3), (3, 3, 8, 8, 3),
                                         (2, 50, 4096, 7, 641), (0, 1, 5, 4, 101)])
def test_reach_is_the_extent_of_what_the_formula_reads(core_exe, off, J, p, q, K):
    r = subprocess.run([core_exe, "reach", str(off), str(J), str(p), str(q), str(K)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    any_, lo, hi = (int(v) for v in r.stdout.split())
    idx = [(off + j * q - k) // p for j in range(J) for k in range((off + j * q) % p, K, p)]
    assert bool(any_) == bool(idx)
    if idx:
        assert (lo, hi) == (min(idx), max(idx))


def test_the_odd_reach_rule_at_its_two_boundaries():
    """p = q = 1, K taps at offset off: output j reads x[j + off - K + 1 .. j + off].  The lowest index is off - K + 1 >= -(T - 1), the highest
    J - 1 + off <= 2 (T - 1): each is taken at the boundary and refused one beyond it (the null pointer is what remains to be reported at the boundary)"""
    L = _lib.lib()
    T = 40
    ok = lambda **kw: L.qdas_resample(C.byref(_desc(T=T, x_ld=T, p=1, q=1, edge=1, **kw)), None, P, P)
    assert ok(K=T, off=0, J=T, out_ld=T) == 1 and "null pointer" in L.qdas_last_error().decode()              # reads x[-(T - 1)]
    assert ok(K=T + 1, off=0, J=T, out_ld=T) == 1 and "reach" in L.qdas_last_error().decode()                  # reads x[-T]
    assert ok(K=1, off=T - 1, J=T, out_ld=T) == 1 and "null pointer" in L.qdas_last_error().decode()          # reads x[2 (T - 1)]
    assert ok(K=1, off=T, J=T, out_ld=T) == 1 and "reach" in L.qdas_last_error().decode()                      # reads x[2 T - 1]
    assert ok(K=1, off=T, J=T - 1, out_ld=T) == 1 and "null pointer" in L.qdas_last_error().decode()
    one = lambda **kw: L.qdas_resample(C.byref(_desc(T=1, x_ld=1, p=1, q=1, edge=1, **kw)), None, P, P)
    assert one(K=1, off=0, J=1) == 1 and "null pointer" in L.qdas_last_error().decode()                        # a record of one sample reflects nowhere
    assert one(K=2, off=0, J=1) == 1 and "reach" in L.qdas_last_error().decode()
    # phases without taps read nothing: p = 8, K = 3, off = 3 meets phase 3 alone
    assert L.qdas_resample(C.byref(_desc(T=2, x_ld=2, p=8, q=8, K=3, off=3, J=1000, out_ld=1000, edge=1)), None, P, P) == 1 and "null pointer" in L.qdas_last_error().decode()


def test_the_stream_travels_in_the_descriptor_and_there_is_no_work_space():
    with open(os.path.join(ROOT, "include", "qdas.h")) as f:
        header = f.read()
    assert not [n for n in stream_entries(header) if "resample" in n or "upfirdn" in n]
    proto = re.search(r"\bint\s+qdas_resample\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1)
    assert "stream" not in proto and "qdas_resample_desc" in proto and proto.count(",") == 3
    assert "queue" in [n for n, _ in _lib.ResampleDesc._fields_]
    from tests import test_gpu_resample as G
    assert callable(G.test_stream_delayed_producer_on_a_side_stream)
    from tests.test_scratch_host import scratch_users
    for fn in ("resample.hip", "resample_core.h"):
        with open(os.path.join(ROOT, "qups_amd", "csrc", fn)) as f:
            src = f.read()
        assert not scratch_users(src) and "hipMalloc" not in src and "Synchronize" not in src and "atomic" not in re.sub(r"//[^\n]*", "", src)
    with open(os.path.join(ROOT, "qups_amd", "csrc", "resample_core.h")) as f:
        assert "hip/" not in f.read(), "the core has no HIP dependency"
    with open(os.path.join(ROOT, "qups_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert " resample.hip" in mk and " resample_core.h" in mk


# ---------------------------------------------------------------------------------------------------------------- the Python layer without a device
def test_python_argument_handling_without_a_device():
    import torch
    for call in (lambda: RS.resample(torch.zeros(8, 2), 3, 2), lambda: RS.resample(np.zeros((8, 2)), 3, 2), lambda: RS.upfirdn([1.0], torch.zeros(8, 2), 2, 1),
                 lambda: RS.filtfilt([0.5, 0.5], torch.zeros(8, 2))):
        with pytest.raises(RS.DasError, match="device tensor"):
            call()
    with pytest.raises(RS.DasError, match=r"more than 3 \(K - 1\) = 9 samples"):
        RS.filtfilt(np.ones(4), torch.zeros(9, 2))
    with pytest.raises(RS.DasError, match="real"):
        RS.filtfilt(np.ones(2) * 1j, torch.zeros(9, 2))
    with pytest.raises(RS.DasError):
        RS.upfirdn([1.0], torch.zeros(8), 0, 1)
    assert np.allclose(RS.filtfilt_taps([1.0, 2.0, 3.0]), [3, 8, 14, 8, 3])


def test_the_rational_choice_and_the_time_axis_rules():
    """62.5 MHz -> 40 MHz is 16/25; an irrational ratio raises and asks for p, q; filtfilt and resample keep t0, fftfilt moves it by (K - 1) / 2 / fs.  The
    device is not reached: each call is stopped at the data (a host tensor on a machine without a device raises RuntimeError, with one it would run)."""
    import torch
    from qups_amd import ChannelData, DasError
    from qups_amd import resample as rs_fn
    seen = {}

    def spy(x, p, q, n=10, beta=5.0, h=None):
        seen["pq"] = (p, q, n, beta)
        return torch.zeros((RS.resample_len(x.shape[0], p, q),) + tuple(x.shape[1:]))

    chd = ChannelData(torch.zeros(50, 3, 2), np.array([1e-6, 2e-6]).reshape(1, 1, 2), 62.5e6)
    mod = importlib.import_module("qups_amd.resample")
    orig, dev = mod.resample, ChannelData._device_data
    try:
        mod.resample = spy
        ChannelData._device_data = lambda self, what: self._torch_data()
        out = chd.resample(40e6)
        assert seen["pq"] == (16, 25, 10, 5.0) and out.fs == 62.5e6 * 16 / 25 == 40e6 and out.t0 is chd.t0 and tuple(out.data.shape) == (32, 3, 2)
        out = chd.resample(0.0, p=6, q=4, n=4)
        assert seen["pq"] == (3, 2, 4, 5.0) and out.fs == 62.5e6 * 1.5 and tuple(out.data.shape) == (75, 3, 2)
        ntm = ChannelData(torch.zeros(3, 50, 2), 0.5e-6, 62.5e6, "NTM").resample(125e6)
        assert seen["pq"][:2] == (2, 1) and ntm.order == "NTM" and tuple(ntm.data.shape) == (3, 100, 2) and ntm.t0 == 0.5e-6 and ntm.fs == 125e6
        with pytest.raises(DasError, match="explicit"):
            chd.resample(62.5e6 * np.sqrt(0.5))
        with pytest.raises(DasError, match="explicit"):
            chd.resample(62.5e6 * 4097 / 4099)
        with pytest.raises(DasError):
            chd.resample(40e6, p=3)
    finally:
        mod.resample, ChannelData._device_data = orig, dev
    assert rs_fn is orig
    with pytest.raises(DasError, match="IIR"):
        chd.filtfilt([1.0, 0.5], a=[1.0, -0.2])
    with pytest.raises(DasError, match="IIR"):
        chd.filtfilt(None, sos=np.ones((1, 6)))
    import inspect
    src = inspect.getsource(ChannelData.fftfilt)
    assert "self.filter(b, dim)" in src, "fftfilt routes to filter: the same result and t0 -= (K - 1) / 2 / fs"
    for m in (ChannelData.resample, ChannelData.filtfilt):
        assert "precision" in m.__doc__
    assert "non-uniform" in ChannelData.resample.__doc__ and "1 %" in ChannelData.resample.__doc__


# ---------------------------------------------------------------------------------------------------------------- the device's core, on the host
@pytest.fixture(scope="module")
def core_exe(tmp_path_factory):
    """resample_core.h under AddressSanitizer and UBSan in a stand-alone program: taps, span and records are heap blocks of exactly their size"""
    exe = str(tmp_path_factory.mktemp("rs") / "resample_core_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "qups_amd", "csrc"), os.path.join(ROOT, "tests", "resample_core_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _fmt(v):
    return " ".join(float(t).hex() for t in np.asarray(v, np.float64).reshape(-1))


TYPES = {"i16": 0, "f32": 1, "c64": 2, "f64": 3, "c128": 4}


def core_data(T, Cn, tname, seed):
    x = _x(T, Cn, tname in ("c64", "c128"), seed)
    if tname == "i16":
        return np.clip(np.round(x * 600), -2000, 2000)
    rt = np.float32 if tname in ("f32", "c64") else np.float64
    return (x.real.astype(rt) + 1j * x.imag.astype(rt)) if np.iscomplexobj(x) else x.astype(rt).astype(np.float64)


def run_core(exe, tmp_path, x, h, p, q, off, J, edge, tname):
    """``(out J x C, geometry line)``; x: T x C in the values the program is to see"""
    T, Cn = x.shape
    cplx = np.iscomplexobj(x)
    path = str(tmp_path / "case.txt")
    with open(path, "w") as f:
        f.write(f"{TYPES[tname]} {int(edge == 'odd')} {T} {Cn} {len(h)} {p} {q} {off} {J}\n")
        f.write(_fmt(h) + "\n")
        flat = np.asarray(x).T.reshape(-1)
        f.write(_fmt(np.stack([flat.real, flat.imag], 1) if cplx else flat) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    geom = dict(zip(("TJ", "lanes", "span", "lds", "loads_max"), (int(v) for v in lines[0].split())))
    val = np.array([complex(float.fromhex(a), float.fromhex(c)) for a, c in (ln.split() for ln in lines[1:])])
    val = val.reshape(Cn, J).T
    return (val if cplx else val.real), geom


def core_case(core_exe, tmp_path, tname, p, q, K, edge, T=None, off=None, J=None, Cn=1):
    dbl = tname in ("f64", "c128")
    rt = np.float64 if dbl else np.float32
    h = (np.random.default_rng(K + p).standard_normal(K) / np.sqrt(-(-K // p))).astype(rt).astype(np.float64)
    off = (K - 1) // 2 if off is None else off
    if edge == "odd":
        T = max(T or 0, K + 2)                                        # the reach: off - (K - 1) >= -(T - 1) and (J - 1) q / p + off / p <= 2 (T - 1)
        J = J or max(1, min(700, ((2 * (T - 1)) * p - off) // q))
    else:
        T = T or max(3, min(1500, (300 * q) // p + 5))
        J = J or R.upfirdn_len(T, K, p, q) + 2
    x = core_data(T, Cn, tname, seed=T + K)
    got, geom = run_core(core_exe, tmp_path, x, h, p, q, off, J, edge, tname)
    want = R.polyphase(h, x, p, q, off, J, edge)
    bd = R.bound(h, p, np.abs(np.concatenate([x.real, x.imag])).max(), double=dbl, odd=edge == "odd")
    err = max(np.abs(got.real - want.real).max(), np.abs(np.imag(got) - np.imag(want)).max())
    print(f"resample core {tname} p/q = {p}/{q}, K = {K}, T = {T}, J = {J}, {edge}: {err / bd:.3f} of the bound, TJ = {geom['TJ']}, span {geom['span']}")
    assert geom["lds"] <= 65536
    assert err <= bd
    return geom


PQ = [(1, 1), (3, 2), (2, 3), (16, 25), (1, 32), (32, 1), (7, 4096), (4096, 7)]


@pytest.mark.parametrize("edge", ["zero", "odd"])
@pytest.mark.parametrize("p,q", PQ)
def test_the_core_on_the_host_matches_the_restatement(core_exe, tmp_path, p, q, edge):
    """K in {1, p - 1, p + 1, 641}, the types in turn so that every type meets every rate class"""
    types = list(TYPES)
    for n, K in enumerate(sorted({1, max(p - 1, 1), p + 1, 641})):
        tname = types[(n + p + q) % 5]
        kw = {}
        if q == 4096:
            kw = dict(T=3 * 4096 // p + 700, J=3 if edge == "zero" else None)
        core_case(core_exe, tmp_path, tname, p, q, K, edge, **kw)


@pytest.mark.parametrize("tname", list(TYPES))
def test_the_core_in_every_type(core_exe, tmp_path, tname):
    core_case(core_exe, tmp_path, tname, 5, 4, 101, "zero", Cn=2)
    core_case(core_exe, tmp_path, tname, 1, 1, 51, "odd", T=3 * 25 + 1, off=25, J=76)                     # filtfilt's shape at its shortest record
    core_case(core_exe, tmp_path, tname, 1, 32, 641, "zero", T=64 * 32 * 2 + 40)                          # the accepted extreme: a 64-output tile


def test_the_core_with_more_taps_than_samples(core_exe, tmp_path):
    for p, q in ((1, 1), (3, 2), (2, 3)):
        core_case(core_exe, tmp_path, "f32", p, q, 129, "zero", T=7)
        core_case(core_exe, tmp_path, "c128", p, q, 641, "zero", T=1)


def test_the_core_stages_each_sample_once_per_tile(core_exe, tmp_path):
    g = core_case(core_exe, tmp_path, "f32", 1, 1, 33, "zero", T=5000, off=16, J=5000)
    assert g["TJ"] == 1024 and g["loads_max"] == 2, "a tile's span overlaps its neighbour's by K - 1 < TJ samples"
    g = core_case(core_exe, tmp_path, "f32", 1, 1, 33, "odd", T=500, off=16, J=500)
    assert g["loads_max"] <= 1 + 1 + 16, "x[0] is also the anchor of its 16 reflected neighbours"


def test_gateway_compiles_and_links():
    """mex/qdas_mex.c with the 'resample' command against the fake MEX API of tests/fake_mex (the run itself needs a GPU: tests/test_mex_resample.py)"""
    from tests import test_mex_resample as M
    exe = M.build_gateway()
    assert os.path.exists(exe)
