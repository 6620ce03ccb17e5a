"""pwznxcorr without a device: the float64 restatement (tests/pwznxcorr_ref.py) pinned to MATLAB's documented ``conv 'same'`` example, to a
sample-by-sample evaluation of the definitions and to the reference's docstring example; argument routing and errors; the layout function;
the C ABI's validation."""
import ctypes as C

import numpy as np
import pytest

from qups_amd import _lib, correlator
from tests import pwznxcorr_ref as R


# ---- the restatement
def test_matlab_conv_same_example():
    """MATLAB's documentation of conv: conv([-1 2 3 -2 0 1 2], [2 4 -1 1], 'same') = [15 5 -9 7 6 7 -1] (numpy's 'same' is shifted by one here)"""
    u, v = [-1, 2, 3, -2, 0, 1, 2], [2, 4, -1, 1]
    assert R.conv_same(np.array(u, float), v).tolist() == [15, 5, -9, 7, 6, 7, -1]
    assert np.convolve(u, v, "same").tolist() != [15, 5, -9, 7, 6, 7, -1]
    assert R.conv_same(np.array(u, float), v).tolist() == np.convolve(u, v, "full")[2:2 + 7].tolist()


def _by_definition(xl, xr, w, lags, zero, norm, pad):
    """every output sample from the definitions, one scalar at a time: (T, N, L)"""
    T, N = xl.shape
    W, h = len(w), len(w) // 2
    P = max(abs(l) for l in lags) if pad else 0
    Tp = T + P
    at = lambda a, i: a[i] if 0 <= i < len(a) else 0.0

    def K(a, s):
        return sum(w[k] * at(a, s + h - k) for k in range(W))
    y = np.zeros((T, N, len(lags)), complex)
    for n in range(N):
        a = list(xl[:, n]) + [0.0] * P
        b = list(xr[:, n]) + [0.0] * P
        xlz = [a[s] - K(a, s) if zero else a[s] for s in range(Tp)]
        pl = [abs(v) ** 2 for v in xlz]
        for i, l in enumerate(lags):
            c = [np.conj(b[(s + l) % Tp]) for s in range(Tp)]
            cz = [c[s] - K(c, s) if zero else c[s] for s in range(Tp)]
            pr = [abs(v) ** 2 for v in cz]
            m = [u * v for u, v in zip(xlz, cz)]
            for s in range(T):
                v = K(m, s)
                if norm:
                    v = v / (np.sqrt(K(pl, s)) * np.sqrt(K(pr, s)))
                y[s, n, i] = v
    return y


@pytest.mark.parametrize("pad", [True, False])
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("zero", [True, False])
@pytest.mark.parametrize("W", [3, 4])
def test_restatement_against_the_definitions(W, zero, norm, pad):
    rng = np.random.default_rng(W)
    x = (rng.standard_normal((24, 4)) + 1j * rng.standard_normal((24, 4))) * (1 + 3 * rng.random((1, 4)))
    w = rng.random(W) + 0.1
    lags = [-2, 0, 3]
    got = R.core(x[:, :3], x[:, 1:], w, lags, zero, norm, pad)
    with np.errstate(invalid="ignore"):
        want = _by_definition(x[:, :3], x[:, 1:], w, lags, zero, norm, pad)
    # (a negative lag with the pad and without debiasing leaves the first windows of the right trace empty: 0 / 0 in both)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * np.nanmax(np.abs(want)), equal_nan=True)
    assert np.isnan(want).sum() <= want.size // 8
    assert np.array_equal(R.pwznxcorr(x, lags, w, zero=zero, norm=norm, pad=pad), got, equal_nan=True)


def test_the_three_consequences_kept_from_the_reference():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((32, 2)) + 3.0
    # a scalar W is ones(W), not a mean: subtracting the window SUM differs from subtracting the window mean
    a, b = R.pwznxcorr(x, [0], 4, norm=False), R.pwznxcorr(x, [0], np.ones(4) / 4, norm=False)
    assert not np.allclose(a, b * 4) and not np.allclose(a, b)
    # the pad region carries -K(xl) and the wrapped samples: the last output times differ from a computation without the pad
    p, q = R.pwznxcorr(x, [2], 5), R.pwznxcorr(x, [2], 5, pad=False)
    assert np.allclose(p[8:20], q[8:20]) and not np.allclose(p[-3:], q[-3:])


def _mode(a):
    return np.array([np.bincount(c).argmax() for c in a.T])


@pytest.mark.parametrize("mean", [False, True])
def test_docstring_example_recovers_the_shifts(mean):
    """kern/pwznxcorr.m's example, scaled down: the per-channel mode of the peak lag is -diff(tn)"""
    rng = np.random.default_rng(0)
    T, N, P = 512, 16, 10
    fc, sig = 2, 2
    fs = P * fc
    tn = rng.integers(-2, 3, N)
    theta = fc * (np.arange(T)[:, None] + tn) / fs
    x = np.sin(2 * np.pi * (theta + 1e-2 * sig * rng.standard_normal(theta.shape)))
    L, W = 5, 50
    y = R.pwznxcorr(x, L, np.ones(W) / W if mean else W)
    assert y.shape == (T, N - 1, 2 * L + 1)
    assert np.array_equal(np.arange(-L, L + 1)[_mode(np.argmax(y, axis=2))], -np.diff(tn))


# ---- argument routing (no device)
def test_lag_expansion_and_default_window():
    assert correlator.expand_lags(3).tolist() == [-3, -2, -1, 0, 1, 2, 3]
    assert correlator.expand_lags([4]).tolist() == list(range(-4, 5))
    assert correlator.expand_lags([3, -1, 3, 0]).tolist() == [3, -1, 3, 0]
    assert correlator.expand_lags(0).tolist() == [0]
    for L, W in ((0, 1), (1, 1), (2, 1), (3, 2), (5, 3), (8, 4)):
        p = correlator.plan((64, 4), L)
        assert p["w"].tolist() == [1.0] * W and p["w"].tolist() == R.window(None, R.expand_lags(L)).tolist()
    assert correlator.plan((64, 4), [7, -9])["w"].size == 5 and correlator.plan((64, 4), [7, -9])["P"] == 9
    assert correlator.plan((64, 4), [7, -9], pad=False)["P"] == 0
    assert correlator.plan((64, 4), 2, 6)["w"].tolist() == [1.0] * 6
    assert correlator.plan((64, 4), 2, [0.5, 0.25])["w"].tolist() == [0.5, 0.25]
    assert correlator.plan((64, 4), 2, np.ones((3, 1)))["w"].size == 3
    assert correlator.plan((4, 64), 2, np.ones((1, 3)), tdim=2, ndim=1)["w"].size == 3


def test_center_channels():
    assert correlator.center_channels(5) == [2]              # channel (N + 1) / 2 = 3, 1-based
    assert correlator.center_channels(6) == [2, 3]           # channels N/2 and N/2 + 1, 1-based
    assert correlator.center_channels(1) == [0] and correlator.center_channels(2) == [0, 1]
    x = np.arange(12.0).reshape(2, 6)
    want = R.core(x, x[:, [2, 3]].mean(1, keepdims=True), np.ones(1), [0], False, False, False)
    assert np.array_equal(R.pwznxcorr(x, [0], 1, zero=False, norm=False, pad=False, ref="center"), want)


def test_output_shapes():
    P = correlator.plan
    assert P((96, 5), 3)["shape"] == (96, 4, 7)
    assert P((96, 5), 3, stride=2)["shape"] == (96, 3, 7)
    assert P((96, 5), 3, ref="center")["shape"] == (96, 5, 7)
    assert P((96, 5, 2), 3, ref="x0", x0_shape=(96,))["shape"] == (96, 5, 2, 7)
    assert P((96, 5, 2), 3, ref="x0", x0_shape=(96, 5, 2))["shape"] == (96, 5, 2, 7)
    assert P((5, 96, 2), 3, tdim=2, ndim=1)["shape"] == (4, 96, 2, 7)
    assert P((96, 5, 1, 3), 2, ldim=3)["shape"] == (96, 4, 5, 3)
    assert P((96, 5, 1, 3), 2, ldim=6)["shape"] == (96, 4, 1, 3, 1, 5)
    assert P((96,), 2, tdim=1, ndim=2, ref="center")["shape"] == (96, 1, 5)
    for kw in ({}, {"stride": 2}, {"ref": "center"}, {"ldim": 3}, {"ldim": 5}):
        x = np.random.default_rng(3).standard_normal((20, 4, 1))
        assert R.pwznxcorr(x, 2, 3, **kw).shape == P(x.shape, 2, 3, **kw)["shape"]


def test_no_pairs_is_an_empty_result_without_a_device(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for N, S in ((1, 1), (3, 3), (3, 5)):
        y = correlator.pwznxcorr(np.ones((16, N), np.float32), 2, stride=S)
        assert tuple(y.shape) == (16, 0, 5) and y.dtype == torch.float32
    assert tuple(correlator.pwznxcorr(np.ones((16, 3), np.complex64), -1).shape) == (16, 2, 0)     # the scalar -1 is the empty list 1:-1
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        correlator.pwznxcorr(np.ones((16, 3), np.float32), 2)


@pytest.mark.parametrize("kw,exc,text", [
    ({"U": 2}, NotImplementedError, "U > 1"),
    ({"U": 0}, ValueError, "U must be a positive integer"),
    ({"lags": [0.5, 1]}, NotImplementedError, "non-integer lags"),
    ({"lags": 1.5}, NotImplementedError, "non-integer lags"),
    ({"multi": True}, NotImplementedError, "multi=True"),
    ({"iflt": True}, NotImplementedError, "iflt=True"),
    ({"W": np.ones((3, 2))}, NotImplementedError, "non-scalar along the channel dimension"),
    ({"W": np.ones((3, 1, 2))}, ValueError, "QUPS:pwznxcorr:incompatibleWeightSize"),
    ({"W": np.ones(3) * 1j}, ValueError, "must be real"),
    ({"W": [1.0, -0.5, 1.0]}, ValueError, "negative weight"),
    ({"W": 0}, ValueError, "positive integer"),
    ({"W": 2.5}, ValueError, "positive integer"),
    ({"ref": "median"}, ValueError, "ref must be one of"),
    ({"ref": "x0"}, ValueError, "needs the reference traces x0"),
    ({"ref": "x0", "x0_shape": (95,)}, ValueError, "time length 96"),
    ({"ref": "x0", "x0_shape": (96, 4)}, ValueError, "1 or equal"),
    ({"stride": 0}, ValueError, "stride must be a positive integer"),
    ({"tdim": 0}, ValueError, "tdim"),
    ({"tdim": 2}, ValueError, "tdim must differ from ndim"),
    ({"ldim": 2}, ValueError, "ldim"),
    ({"ldim": 3}, ValueError, "names a dimension of x of size 2"),
])
def test_rejected_options(kw, exc, text):
    kw = dict(kw)
    lags = kw.pop("lags", 3)
    with pytest.raises(exc, match=text):
        correlator.plan((96, 5, 2), lags, **kw)


def test_a_negative_weight_is_accepted_without_norm_and_lvec_is_ignored():
    assert correlator.plan((96, 5), 3, [1.0, -0.5], norm=False)["w"].tolist() == [1.0, -0.5]
    assert correlator.plan((96, 5), 3, lvec=False)["shape"] == correlator.plan((96, 5), 3, lvec=True)["shape"]
    with pytest.raises(ValueError, match="floating-point"):
        correlator.pwznxcorr(np.ones((8, 3), np.int32), 1)


# ---- the layout decision
def test_layout_of_the_das_view():
    """DAS(keep_rx=True): I1 x I2 x I3 x F x N x 1 with I1 fastest; depth is time, N the channels: the rest is one batch group, no copy"""
    I1, I2, I3, F, N = 40, 30, 1, 2, 16
    shape = (I1, I2, I3, F, N, 1)
    strides = (1, I1, I1 * I2, I1 * I2 * I3, I1 * I2 * I3 * F, I1 * I2 * I3 * F * N)
    groups, order = correlator.record_layout(shape, strides, 0, 4)
    assert groups == [(I2 * F, I1, (), 1), (1, 0, (), None)] and order == [1, 3]


def test_layouts_that_need_a_copy_and_batch_groups():
    L = correlator.record_layout
    assert L((96, 5), (5, 1), 0, 1) is None                                  # torch row-major T x N: time is not contiguous
    assert L((96, 5), (1, 96), 0, 1) == ([(1, 0, (), None)] * 2, [])
    assert L((5, 96, 2), (96, 1, 480), 1, 0) == ([(2, 480, (), 2), (1, 0, (), None)], [2])
    # two batch dimensions that do not continue each other: two groups; a third: a copy
    assert L((96, 4, 3, 2), (1, 96, 768, 1920), 0, 1) == ([(3, 768, (), 2), (2, 1920, (), 3)], [2, 3])
    assert L((96, 4, 3, 2, 2), (1, 96, 768, 1920, 5000), 0, 1) is None
    # a second operand: one trace for all (strides 0) merges like x; one trace per entry of the slower batch dimension splits the group
    sh, st = (96, 5, 3, 2), (1, 96, 480, 1440)
    assert L(sh, st, 0, 1, [(1, 0, 0, 0)]) == ([(6, 480, (0,), 2), (1, 0, (0,), None)], [2, 3])
    assert L(sh, st, 0, 1, [(1, 0, 0, 96)]) == ([(3, 480, (0,), 2), (2, 1440, (96,), 3)], [2, 3])
    assert L(sh, st, 0, 1, [(2, 0, 0, 0)]) is None                           # the other operand's time is strided
    assert L((1, 5, 3), (7, 1, 5), 0, 1) is not None                         # a single sample: any time stride


# ---- the C ABI
def _desc(**kw):
    d = _lib.PwznxcorrDesc()
    d.dtype, d.cplx, d.device, d.zero, d.norm, d.pad = _lib.QDAS_F32, 1, -1, 1, 1, 1
    d.T, d.N, d.W, d.nlags = 96, 4, 8, 3
    d.bsize[0], d.bsize[1] = 1, 1
    d.xl_strideN = d.xr_strideN = d.y_strideN = 96
    d.y_strideL = 96 * 4
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_abi_symbol_struct_and_constants():
    L = _lib.lib()
    assert "qdas_pwznxcorr" in _lib.SYMBOLS and hasattr(L, "qdas_pwznxcorr")
    assert C.sizeof(_lib.PwznxcorrDesc) == 152               # 6 int32 + 6 uint64 + 10 int64 (include/qdas.h)
    assert L.qdas_pwznxcorr_time_tile() == correlator.TIME_TILE == 256
    assert L.qdas_version() == 103
    for dt, isz in ((_lib.QDAS_F32, 4), (_lib.QDAS_F64, 8)):
        for cplx in (0, 1):
            for W, span in ((1, 0), (64, 16), (256, 512), (300, 7)):
                assert L.qdas_pwznxcorr_lds_bytes(dt, cplx, W, span) == correlator.lds_bytes(isz, bool(cplx), W, span)
    assert correlator.lds_bytes(8, True, 256, 512) == 53144 <= correlator.LDS_LIMIT


def test_abi_validation_needs_no_device():
    L = _lib.lib()
    buf, lags = C.c_void_p(1), (C.c_int64 * 3)(-1, 0, 1)
    call = lambda d, xl=buf, xr=buf, w=buf, lg=lags, y=buf: L.qdas_pwznxcorr(C.byref(d) if d is not None else None, xl, xr, w, lg, y, None)
    assert call(None) == 1 and b"null descriptor" in L.qdas_last_error()
    assert call(_desc(dtype=_lib.QDAS_F16)) == 1 and b"double or single" in L.qdas_last_error()
    assert call(_desc(W=0)) == 1 and b"W = 0" in L.qdas_last_error()
    assert call(_desc(), lg=None) == 1 and b"null lag table" in L.qdas_last_error()
    assert call(_desc(), xl=None) == 1 and b"null data pointer" in L.qdas_last_error()
    assert call(_desc(), w=None) == 1 and b"null data pointer" in L.qdas_last_error()
    big = (C.c_int64 * 3)(-1, 0, 40000)
    assert call(_desc(), lg=big) == 2 and b"32767" in L.qdas_last_error()
    many = (C.c_int64 * (correlator.MAX_LAGS + 1))()
    assert call(_desc(nlags=correlator.MAX_LAGS + 1), lg=many) == 2 and b"lags per call" in L.qdas_last_error()
    assert call(_desc(dtype=_lib.QDAS_F64, W=2000)) == 2 and b"LDS" in L.qdas_last_error()
    wide = (C.c_int64 * 2)(-20000, 20000)
    assert call(_desc(nlags=2), lg=wide) == 2 and b"LDS" in L.qdas_last_error()
    assert call(_desc(T=1 << 30)) == 2
    assert call(_desc(N=1 << 20, T=1 << 20)) == 2 and b"workgroups" in L.qdas_last_error()


def test_abi_empty_results_launch_nothing():
    """T, N, a batch size or nlags = 0: the arguments are still validated, nothing is launched (no device needed), NULL data is fine"""
    L = _lib.lib()
    lags = (C.c_int64 * 3)(-1, 0, 1)
    for kw in ({"T": 0}, {"N": 0}, {"nlags": 0}):
        assert L.qdas_pwznxcorr(C.byref(_desc(**kw)), None, None, None, lags, None, None) == 0, L.qdas_last_error()
    d = _desc()
    d.bsize[1] = 0
    assert L.qdas_pwznxcorr(C.byref(d), None, None, None, lags, None, None) == 0
    assert L.qdas_pwznxcorr(C.byref(_desc(T=0, W=0)), None, None, None, lags, None, None) == 1
