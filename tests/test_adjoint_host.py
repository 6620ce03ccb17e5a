"""Host side of the adjoint beamformer (no device): the float64 restatement (tests/adjoint_ref.py) pinned by facts that follow from the formulas, the
frequency selection, ``Sequence.t0Offset``, the routing of the apodization classes, the C ABI's symbol, descriptor and validation, argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch

from qups_amd import ChannelData, DasError, Scan, Sequence, Transducer, UltrasoundSystem, _lib
from qups_amd import adjoint as A
from tests import adjoint_ref as R

FS, C0, FC = 20e6, 1540.0, 5e6


def _point_target(seq_kind, T=512):
    """12 elements at 0.3 mm, a point target at (0.2, 0, 10) mm, a 21 x 21 grid at 0.1 mm centred on it"""
    N = 12
    Pe = np.stack([(np.arange(N) - (N - 1) / 2) * 0.3e-3, np.zeros(N), np.zeros(N)])
    sc = np.array([0.2e-3, 0.0, 10e-3])
    gx, gz = sc[0] + np.arange(-10, 11) * 0.1e-3, sc[2] + np.arange(-10, 11) * 0.1e-3
    Z, Xg = np.meshgrid(gz, gx, indexing="ij")
    Pi = np.stack([Xg.ravel(order="F"), np.zeros(Xg.size), Z.ravel(order="F")])
    rx = np.linalg.norm(Pe - sc[:, None], axis=0) / C0
    if seq_kind == "FSA":
        del_tx, apod_tx = np.zeros((N, N)), np.eye(N)
    else:                                                    # seq.delays-style steering: element m fires at del_tx[m, v] = -(n_v . p_m) / c0
        th = np.deg2rad(np.linspace(-8, 8, 5))
        nv = np.stack([np.sin(th), 0 * th, np.cos(th)])
        del_tx, apod_tx = -(nv[:, None, :] * Pe[:, :, None]).sum(0) / C0, np.ones((N, 5))
    t = np.arange(T)[:, None, None] / FS
    x = 0
    for m in range(N):                                       # every element's wave, scattered once, as each receiver sees it
        d = rx[None, :, None] + (rx[m] + del_tx[m])[None, None, :]
        x = x + apod_tx[m][None, None, :] * np.exp(-0.5 * ((t - d) / 0.2e-6) ** 2) * np.exp(2j * np.pi * FC * (t - d))
    return x, Pi, Pe, del_tx, apod_tx, (10 + 21 * 10)          # the scatterer's pixel: row 10 of column 10


# ---------------------------------------------------------------------------------------------------------------- (a), (b): the restatement
def test_fsa_norm_is_sqrt_m_and_b_is_the_direct_triple_sum():
    rng = np.random.default_rng(0)
    N = M = 6
    K = 16
    Pe = np.stack([(np.arange(N) - 2.5) * 0.3e-3, np.zeros(N), np.zeros(N)])
    Pi = np.stack([rng.uniform(-1e-3, 1e-3, 9), np.zeros(9), rng.uniform(5e-3, 9e-3, 9)])
    cinv = np.full(9, 1 / C0)
    X = rng.standard_normal((K, N, M)) + 1j * rng.standard_normal((K, N, M))
    tau = R.delays(Pe, Pi, cinv)
    for k in (1, 5):
        A_ = R.transmit_field(k * FS / K, tau, np.zeros((M, M)), np.eye(M))
        assert np.allclose(np.linalg.norm(A_, axis=1), np.sqrt(M), rtol=1e-13)
    bins = np.arange(K // 2)
    b = R.adjoint(X, bins, FS, Pi, Pe, Pe, cinv, np.zeros((M, M)), np.eye(M))
    f = bins * FS / K
    Grx = np.exp(2j * np.pi * f[:, None, None] * tau[None])                       # k x i x n
    direct = np.einsum("kin,knv,kiv->i", Grx, X[bins], Grx) / np.sqrt(M)         # tau_tx = tau_rx here
    assert np.allclose(b, direct, rtol=1e-11, atol=1e-11 * np.abs(direct).max())


@pytest.mark.parametrize("kind", ["FSA", "PW"])
def test_point_target_lands_on_its_pixel(kind):
    x, Pi, Pe, del_tx, apod_tx, pix = _point_target(kind)
    X = R.spectrum(x, 0.0, FS)
    b = R.adjoint(X, R.select_bins(X, FS), FS, Pi, Pe, Pe, np.full(Pi.shape[1], 1 / C0), del_tx, apod_tx)
    assert int(np.argmax(np.abs(b))) == pix


def test_kept_dimensions_sum_to_the_image():
    x, Pi, Pe, del_tx, apod_tx, _ = _point_target("PW", T=64)
    X = R.spectrum(x, 1e-6, FS, fmod=1e6)
    args = (X, R.select_bins(X, FS), FS, Pi[:, :50], Pe, Pe, np.full(50, 1 / C0), del_tx, apod_tx)
    b = R.adjoint(*args)
    for kw, ax in (({"keep_tx": True}, 1), ({"keep_rx": True}, 1), ({"keep_tx": True, "keep_rx": True}, (1, 2))):
        assert np.allclose(R.adjoint(*args, **kw).sum(axis=ax), b, rtol=1e-10, atol=1e-12 * np.abs(b).max())


# ---------------------------------------------------------------------------------------------------------------- (c) frequency selection
def test_fthresh_selection_on_a_hand_made_spectrum():
    K = 16
    X = np.full((K, 2, 3), 1e-6 + 0j)
    X[2, 0, 0] = 1.0                     # the maximum of trace (0, 0)
    X[3, 0, 0] = 0.2                     # -14 dB
    X[5, 1, 2] = 1e-6 * 10 ** 0.5        # trace (1, 2) is flat but for this: its own maximum
    X[9, 0, 0] = 1.0                     # above fs / 2
    X[8, 0, 0] = 1.0                     # f = fs / 2 itself
    for sel in (R.select_bins, lambda X_, fs, th: A.select_bins(torch.from_numpy(X_), fs, th)):
        assert list(sel(X, FS, -np.inf)) == list(range(8))          # without a threshold only the fs / 2 cut acts (bins 8 and 9 hold maxima)
    Y = X.copy()
    Y[0] = 1.0                           # every trace has its maximum in bin 0
    Y[2, 0, 0] = 1.0
    Y[3, 0, 0] = 0.2
    Y[5, 1, 2] = 0.05
    Y[8:] = 1.0
    for sel in (R.select_bins, lambda X_, fs, th: A.select_bins(torch.from_numpy(X_), fs, th)):
        assert list(sel(Y, FS, -3.0)) == [0, 2]
        assert list(sel(Y, FS, -20.0)) == [0, 2, 3]
        assert list(sel(Y, FS, -30.0)) == [0, 2, 3, 5]
        assert max(sel(Y, FS, -200.0)) == 7


def test_spectrum_matches_the_restatement_and_rejects_short_nfft():
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((40, 3, 4)) + 1j * rng.standard_normal((40, 3, 4))).astype(np.complex64)
    t0, off = 3e-6 + rng.uniform(0, 1e-6, 4), -rng.uniform(5e-6, 6e-6, 4)
    for K in (40, 64):
        got = A.spectrum(torch.from_numpy(x), t0, FS, 2.5e6, K, off).numpy()
        ref = R.spectrum(x, t0, FS, 2.5e6, K, off)
        assert got.dtype == np.complex64 and np.abs(got - ref).max() <= 2e-6 * np.abs(ref).max()
    with pytest.raises(DasError, match="Nfft"):
        A.spectrum(torch.from_numpy(x), t0, FS, 0.0, 39)


# ---------------------------------------------------------------------------------------------------------------- (d) t0Offset
def test_t0_offset_per_sequence_type():
    foc = np.array([[0.0, 3e-3], [0.0, 0.0], [4e-3, 4e-3]])
    r = np.array([4e-3, 5e-3]) / C0
    assert np.array_equal(Sequence("FSA", None, C0).t0Offset(), [0.0])
    assert np.array_equal(Sequence("PW", foc, C0).t0Offset(), [0.0])
    for t, sign in (("FC", -1), ("VS", -1), ("DV", 1)):
        assert np.allclose(Sequence(t, foc, C0).t0Offset(), sign * r, rtol=1e-15)
        assert np.allclose(R.t0_offset(t, foc, C0), sign * r, rtol=1e-15)


# ---------------------------------------------------------------------------------------------------------------- (e) apodization routing
def test_apodization_routing_and_the_rejected_shape():
    rng = np.random.default_rng(2)
    Isz, N, V = (4, 3, 1), 5, 2
    an, am, amn = rng.uniform(size=(4, 3, 1, 5)), rng.uniform(size=(4, 1, 1, 1, 2)), rng.uniform(size=(1, 1, 1, 5, 2))
    a_n, a_m, a_mn = A.classify_apods([an], Isz, N, V)
    assert a_m is None and a_mn is None and np.array_equal(a_n, an)
    a_n, a_m, a_mn = A.classify_apods([am], Isz, N, V)
    assert a_n is None and a_mn is None and np.array_equal(a_m, np.broadcast_to(am[:, :, :, 0, :], (4, 3, 1, 2)))
    a_n, a_m, a_mn = A.classify_apods([amn, an, an], Isz, N, V)
    assert a_m is None and np.array_equal(a_mn, amn[0, 0, 0]) and np.array_equal(a_n, an * an)
    a_n, a_m, a_mn = A.classify_apods([np.float64(0.5)], Isz, N, V)                   # a scalar: scalar image dimensions
    assert a_n is None and a_m is None and np.array_equal(a_mn, np.full((5, 2), 0.5))
    with pytest.raises(DasError) as e:
        A.classify_apods([an, rng.uniform(size=(4, 3, 1, 5, 2))], Isz, N, V)
    assert str(e.value).startswith("Unable to apply apodization (2) due to size constraints. Apodization must be scalar in the transmit dimension, "
                                   "receive dimension, or all image dimensions.")
    with pytest.raises(DasError, match="broadcast"):
        A.classify_apods([np.ones((4, 2, 1, 5))], Isz, N, V)


# ---------------------------------------------------------------------------------------------------------------- (f) ABI
def test_abi_symbol_and_descriptor():
    assert "qdas_adjoint" in _lib.SYMBOLS and hasattr(_lib.lib(), "qdas_adjoint")
    D = _lib.AdjointDesc
    assert C.sizeof(D) == 136                                 # 5 extents, 4 pointers, a count, 5 pointers, 4 ints
    assert (D.Pi.offset, D.cinv_count.offset, D.freq.offset, D.a_m.offset, D.keep_rx.offset, D.device.offset) == (40, 72, 80, 112, 120, 132)


# ---------------------------------------------------------------------------------------------------------------- (g) argument errors
def _desc(**kw):
    d = _lib.AdjointDesc()
    d.I, d.N, d.M, d.V, d.Ksel, d.cinv_count, d.dtype, d.device = 8, 4, 4, 2, 3, 1, _lib.QDAS_F32, -1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("kw,code,text", [
    (dict(dtype=_lib.QDAS_F16), 2, "complex64"), (dict(dtype=_lib.QDAS_F64), 2, "complex64"), (dict(dtype=7), 1, "dtype"),
    (dict(keep_rx=2), 1, "keep_rx"), (dict(cinv_count=3), 1, "cinv"), (dict(N=1 << 31), 2, "extent"),
])
def test_c_abi_rejects_bad_descriptors_before_any_launch(kw, code, text):
    L = _lib.lib()
    assert L.qdas_adjoint(C.byref(_desc(**kw)), None, None, None) == code
    assert text in L.qdas_last_error().decode()


def test_c_abi_null_descriptor_and_empty_image():
    L = _lib.lib()
    assert L.qdas_adjoint(None, None, None, None) == 1
    assert L.qdas_adjoint(C.byref(_desc(I=0, cinv_count=0)), None, None, None) == 0       # no pixels: nothing to do, no device needed
    assert L.qdas_adjoint(C.byref(_desc(N=0, keep_rx=1)), None, None, None) == 0


def test_bfadjoint_argument_errors():
    xdc = Transducer.linear(4, 0.3e-3)
    us = UltrasoundSystem(xdc, Sequence("FSA", None, C0, 4), Scan.cartesian(np.linspace(-1e-3, 1e-3, 3), np.linspace(5e-3, 6e-3, 4)), fs=FS)
    x = torch.zeros((16, 4, 4), dtype=torch.complex64)
    with pytest.raises(DasError, match="float32"):
        us.bfAdjoint(ChannelData(x.real.clone(), 0.0, FS))
    with pytest.raises(DasError, match="complex128"):
        us.bfAdjoint(ChannelData(x.to(torch.complex128), 0.0, FS))
    with pytest.raises(DasError, match="Nfft"):
        us.bfAdjoint(ChannelData(x, 0.0, FS), Nfft=8)
    with pytest.raises(DasError, match="receives"):
        us.bfAdjoint(ChannelData(x[:, :3], 0.0, FS))
    with pytest.raises(DasError, match="transmits"):
        us.bfAdjoint(ChannelData(x[:, :, :3], 0.0, FS))
    with pytest.raises(DasError, match="c0"):
        us.bfAdjoint(ChannelData(x, 0.0, FS), c0=np.ones((2, 2)))
    with pytest.raises(DasError, match=r"Unable to apply apodization \(1\)"):
        us.bfAdjoint(ChannelData(x, 0.0, FS), np.ones((4, 3, 1, 4, 4)))
