"""slsc / dmas / cohfac / pcf without a device: the float64 restatement (tests/coherence_ref.py) pinned to closed forms that do not depend
on it, the stride-grouping function that maps tensors onto qdas_coherence's canonical layout, argument errors, and the C ABI's validation."""
import ctypes as C

import numpy as np
import pytest

from qups_amd import _lib, coherence
from tests import coherence_ref as R


def _coherent(N=12, c=1.7 * np.exp(0.4j), shape=(3, 5)):
    return np.broadcast_to(c, shape + (N,)).copy()


@pytest.mark.parametrize("method", ["average", "ensemble"])
def test_fully_coherent_slsc_is_one(method):
    z = R.slsc(_coherent(), 2, method=method)
    assert z.shape == (3, 5, 1)
    np.testing.assert_allclose(z, 1.0, atol=1e-12)


def test_fully_coherent_cohfac_and_pcf():
    x = _coherent()
    np.testing.assert_allclose(R.cohfac(x, 2), 1.0, atol=1e-12)
    w, sf = R.pcf(x, 2)
    np.testing.assert_allclose(w, 1.0, atol=1e-12)
    np.testing.assert_allclose(sf, 0.0, atol=1e-12)


def test_lag_zero_counts_the_diagonal_once():
    """L = [0 5] on a fully coherent x: lag 0 weighs 1/(2L), lag 5 weighs 1/L -> 3/4 (the OpenCL kernel of the reference gives 1)"""
    np.testing.assert_allclose(R.slsc(_coherent(N=16), 2, L=[0, 5]), 0.75, atol=1e-12)


def test_all_zero_pixel_gives_nan_in_the_ensemble_estimator():
    """nan2zero applies to rsqrt(a) rsqrt(b) only: a = b = 0 gives Inf, and the zero inner product times Inf is NaN (MATLAB)"""
    z = R.slsc(np.zeros((2, 6), np.complex128), 1, method="ensemble")
    assert np.all(np.isnan(z))


def test_constant_dmas():
    N, c = 9, 0.8 * np.exp(1.1j)
    b = R.dmas_compress(R.dmas(_coherent(N=N, c=c), 2))
    np.testing.assert_allclose(b, np.exp(2j * np.angle(c)) * abs(c) * np.sqrt(N * (N - 1) / 2), rtol=1e-12)


# ---- the layout mapping
def test_groups_of_the_das_view():
    """DAS(..., keep_rx=True) returns I1 x I2 x I3 x F x N with I1 stride 1 and N stride I1 I2 I3 F: one merged pixel group, no copy"""
    I1, I2, I3, F, N = 40, 30, 1, 2, 16
    shape = (I1, I2, I3, F, N)
    strides = (1, I1, I1 * I2, I1 * I2 * I3, I1 * I2 * I3 * F)
    groups, order = coherence.pixel_groups(shape, strides, [4])
    assert groups == [(I1 * I2 * F, 1), (1, 0), (1, 0)]
    assert order == [0, 1, 2, 3]


def test_groups_of_a_contiguous_pixel_fastest_tensor_with_kdim():
    # torch row-major N x K x I2 x I1 viewed as I1 x I2 x K x N: pixels first, time kernel K at its own stride
    I1, I2, K, N = 7, 5, 3, 11
    shape, strides = (I1, I2, K, N), (1, I1, I1 * I2, I1 * I2 * K)
    groups, _ = coherence.pixel_groups(shape, strides, [3, 2])
    assert groups == [(I1 * I2, 1), (1, 0), (1, 0)]


def test_groups_of_odd_strides_and_the_aperture_fastest_case():
    # every second column of a 10 x 8 x N image: two pixel groups that keep their strides
    shape, strides = (10, 4, 6), (1, 20, 80)
    groups, order = coherence.pixel_groups(shape, strides, [2])
    assert groups == [(10, 1), (4, 20), (1, 0)] and order == [0, 1]
    # a contiguous ... x N tensor (torch row-major, aperture fastest): not expressible -> the wrapper transposes
    assert coherence.pixel_groups((10, 4, 6), (24, 6, 1), [2]) is None
    assert coherence._dense_reduced_first((10, 4, 6), (24, 6, 1), [2]) == (40, 6)
    # more than three pixel groups
    assert coherence.pixel_groups((2, 2, 2, 2, 3), (1, 4, 16, 64, 256), [4]) is None


# ---- argument errors (raised before any device is needed)
def test_pcf_needs_complex_input():
    with pytest.raises(ValueError, match="Input must be complex"):
        coherence.pcf(np.ones((4, 8)), 2)


@pytest.mark.parametrize("fn", [coherence.slsc, coherence.dmas, coherence.cohfac, coherence.pcf])
def test_dims_out_of_range(fn):
    x = np.ones((4, 8), np.complex64)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError):
            fn(x, bad)


def test_empty_and_bad_lag_sets():
    x = np.ones((4, 8), np.complex64)
    for L in ([], 0, [-1, 2], [1.5, 2]):
        with pytest.raises(ValueError):
            coherence.slsc(x, 2, L)
        with pytest.raises(ValueError):
            coherence.dmas(x, 2, L)
    with pytest.raises(ValueError):
        coherence.slsc(x, 2, 1, "bogus")
    with pytest.raises(ValueError):
        coherence.slsc(x, 2, 1, "average", 2)
    with pytest.raises(ValueError):
        coherence.cohfac(x, [2, 2])


def test_lag_specs():
    assert coherence._lag_spec(5, "t") == ("range", 1, 5)
    assert coherence._lag_spec([0, 1, 2], "t") == ("range", 0, 2)
    kind, t = coherence._lag_spec([0, 5], "t")
    assert kind == "table" and t.tolist() == [0, 5]
    kind, t = coherence._lag_spec([3, 3, 4], "t")
    assert kind == "table" and t.tolist() == [3, 3, 4]


def test_no_device_means_no_fallback(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        coherence.slsc(np.ones((4, 8), np.complex64))


# ---- the C ABI validates before any HIP call
def test_coherence_abi_validation_needs_no_device():
    L = _lib.lib()
    d = _lib.CoherenceDesc()
    d.method, d.dtype, d.cplx, d.device, d.N, d.K = 9, _lib.QDAS_F32, 1, -1, 8, 1
    d.size[0], d.stride[0], d.strideN, d.lag_lo, d.lag_hi = 16, 1, 16, 1, 2
    d.size[1], d.size[2] = 1, 1
    buf = C.c_void_p(1)
    assert L.qdas_coherence(C.byref(d), buf, buf, None, None) == 1 and b"unknown method" in L.qdas_last_error()
    d.method = _lib.COH_SLSC_AVERAGE
    d.N = 0
    assert L.qdas_coherence(C.byref(d), buf, buf, None, None) == 1 and b"N = 0" in L.qdas_last_error()
    d.N = 8
    assert L.qdas_coherence(C.byref(d), None, buf, None, None) == 1 and b"null data pointer" in L.qdas_last_error()
    assert L.qdas_coherence(None, buf, buf, None, None) == 1 and b"null descriptor" in L.qdas_last_error()
    d.lag_lo, d.lag_hi = 3, 2
    assert L.qdas_coherence(C.byref(d), buf, buf, None, None) == 1 and b"empty lag set" in L.qdas_last_error()
    d.lag_lo, d.lag_hi = 1, 2
    d.method, d.cplx = _lib.COH_PCF, 0
    assert L.qdas_coherence(C.byref(d), buf, buf, buf, None) == 1 and b"Input must be complex" in L.qdas_last_error()
    d.cplx = 1
    assert L.qdas_coherence(C.byref(d), buf, buf, None, None) == 1 and b"null data pointer" in L.qdas_last_error()
    d.method, d.dtype = _lib.COH_DMAS, _lib.QDAS_F16
    assert L.qdas_coherence(C.byref(d), buf, buf, None, None) == 1 and b"double or single" in L.qdas_last_error()
    d.dtype = _lib.QDAS_F32
    t = (C.c_int64 * 2)(4, -1)
    d.lags, d.nlags = C.cast(t, C.POINTER(C.c_int64)), 2
    assert L.qdas_coherence(C.byref(d), buf, buf, None, None) == 1 and b"non-negative" in L.qdas_last_error()


def test_coherence_abi_empty_image_launches_nothing():
    """a pixel-group size of 0 is an empty image: arguments are still validated, nothing is launched (no device needed), NULL data is fine"""
    L = _lib.lib()
    d = _lib.CoherenceDesc()
    d.method, d.dtype, d.cplx, d.device, d.N, d.K = _lib.COH_SLSC_AVERAGE, _lib.QDAS_F32, 1, -1, 8, 1
    d.size[0], d.size[1], d.size[2], d.stride[0], d.stride[1], d.strideN, d.lag_lo, d.lag_hi = 37, 0, 1, 1, 37 * 8, 37, 1, 2
    for m in (_lib.COH_SLSC_AVERAGE, _lib.COH_SLSC_ENSEMBLE, _lib.COH_DMAS, _lib.COH_COHFAC, _lib.COH_PCF):
        d.method = m
        assert L.qdas_coherence(C.byref(d), None, None, None, None) == 0, L.qdas_last_error()
    d.method, d.lag_lo, d.lag_hi = _lib.COH_SLSC_AVERAGE, 3, 2
    assert L.qdas_coherence(C.byref(d), None, None, None, None) == 1 and b"empty lag set" in L.qdas_last_error()
