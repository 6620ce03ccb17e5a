"""Host side of the migration beamformer (no device): the float64 restatement (tests/migration_ref.py) pinned by facts that follow from the formulas
and by the reference's point-target test, the axes and the Stolt index of ``qups_amd.migration``, argument errors, warnings, and the C ABI's symbol,
descriptor and validation."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from qups_amd import ChannelData, DasError, Scan, Sequence, Transducer, UltrasoundSystem, _lib
from qups_amd import migration as MG
from tests import migration_ref as R

FS, C0, PITCH, T0 = 20e6, 1540.0, 0.3e-3, 1.3e-6
ANG = (-3.0, 0.0, 5.0)


def _case(T=40, N=10, M=3, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, N, M)) + 1j * rng.standard_normal((T, N, M))
    elem = np.stack([(np.arange(N) - (N - 1) / 2) * PITCH, np.zeros(N), np.zeros(N)])
    return x, R.pw_delays(elem, ANG[:M], C0), R.gamma(ANG[:M])


def _mig(x, tau, gam, **kw):
    return R.migrate(x, T0, FS, tau, gam, PITCH, C0, **kw)


# ---------------------------------------------------------------------------------------------------------------- the restatement
def test_linear_in_the_data():
    x, tau, gam = _case()
    y = _case(seed=1)[0]
    a, b = 0.7 - 0.2j, -1.3 + 0.5j
    lhs = _mig(a * x + b * y, tau, gam, Nfft=(48, 12))
    rhs = a * _mig(x, tau, gam, Nfft=(48, 12)) + b * _mig(y, tau, gam, Nfft=(48, 12))
    assert np.allclose(lhs, rhs, rtol=1e-11, atol=1e-12 * np.abs(rhs).max())


def test_kept_transmits_sum_to_the_image():
    x, tau, gam = _case()
    for kw in (dict(), dict(Nfft=(64, 16), fmod=2.5e6, interp="lanczos3")):
        b = _mig(x, tau, gam, **kw)
        bm = _mig(x, tau, gam, keep_tx=True, **kw)
        assert bm.shape == b.shape + (3,) and np.allclose(bm.sum(axis=2), b, rtol=1e-12, atol=1e-13 * np.abs(b).max())


def test_nfft_defaults_to_the_data_size():
    x, tau, gam = _case()
    assert np.array_equal(_mig(x, tau, gam), _mig(x, tau, gam, Nfft=(40, 10)))
    assert _mig(x, tau, gam, Nfft=(32, 8)).shape == (32, 8) and _mig(x, tau, gam, Nfft=(64, 16)).shape == (40, 10)


def test_jacobian_is_the_stated_factor_of_the_spectrum():
    x, tau, gam = _case()
    X = R.spectrum(x, T0, FS, tau)
    F, K = X.shape[:2]
    f, kx = R.axes(F, K, FS, PITCH)
    cs = C0 / np.sqrt(2)
    fkz = cs * np.sign(f)[:, None] * np.sqrt(kx[None, :] ** 2 + f[:, None] ** 2 / cs ** 2)
    fac = (f[:, None] / cs) / (fkz + np.finfo(float).eps)
    on, off = R.resample(X, FS, PITCH, C0, "cubic", True), R.resample(X, FS, PITCH, C0, "cubic", False)
    assert np.allclose(on, off * fac[:, :, None, None], rtol=1e-13, atol=0)
    assert np.all(on[F // 2] == 0)                                       # the f = 0 row: kz = 0


def test_single_column_is_an_integer_index_copy():
    """N = K = 1: kx = 0 only, kkz = j exactly, so every interpolator copies the spectrum of the trace (inside its support)"""
    x, tau, gam = _case(T=33, N=1, M=1)
    kkz = R.stolt_indices(33, 1, FS, PITCH, C0)
    assert np.array_equal(kkz[:, 0], np.arange(33.0))
    X = R.spectrum(x, T0, FS, tau)
    for interp, lo, hi in (("nearest", 0, 33), ("linear", 0, 32), ("cubic", 1, 31), ("lanczos3", 1, 31)):
        y = R.resample(X, FS, PITCH, C0, interp, False)
        assert np.allclose(y[lo:hi], X[lo:hi], rtol=0, atol=1e-15 * np.abs(X).max()) and np.all(y[:lo] == 0) and np.all(y[hi:] == 0)


def _psf():
    N, T = 32, 512
    elem = np.stack([(np.arange(N) - (N - 1) / 2) * PITCH, np.zeros(N), np.zeros(N)])
    ang, scat, t0 = (-5.0, 0.0, 5.0), np.array([2e-3, 0.0, 15e-3]), 12e-6
    return N, T, elem, ang, scat, t0, R.gaussian_echoes(T, elem, ang, scat, t0, FS, C0)


def test_point_target_lands_within_1p1_mm():
    """reference test/BFTest.m:306-316"""
    N, T, elem, ang, scat, t0, x = _psf()
    b = R.migrate(x, t0, FS, R.pw_delays(elem, ang, C0), R.gamma(ang), PITCH, C0, (2 * T, 4 * N))
    xa, za = R.bscan_axes(T, N, 2 * T, 4 * N, t0, FS, C0, PITCH, elem[0, 0])
    assert b.shape == (T, N) and np.abs(b).max() > 0
    iz, ix = np.unravel_index(np.argmax(np.abs(b)), b.shape)
    assert np.hypot(xa[ix] - scat[0], za[iz] - scat[2]) <= 1.1e-3


# ---------------------------------------------------------------------------------------------------------------- axes, gamma, the Stolt index
@pytest.mark.parametrize("F,K", [(64, 16), (96, 24), (60, 20), (77, 18), (34, 12), (8192, 8)])
def test_axes_and_stolt_indices_match_the_reference_expressions(F, K):
    f, kx = MG.axes(F, K, FS, PITCH)
    assert np.array_equal(f, (np.arange(F) - np.floor(F / 2)) / F * FS) and np.array_equal(kx, (np.arange(K) - np.floor(K / 2)) / K / PITCH)
    kkz, ref = MG.stolt_indices(F, K, FS, PITCH, C0), R.stolt_indices_reference(F, K, FS, PITCH, C0)
    assert kkz.shape == (F, K) and np.abs(kkz - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    assert np.array_equal(kkz, R.stolt_indices(F, K, FS, PITCH, C0))
    assert np.array_equal(kkz[:, K // 2], np.arange(F, dtype=float))      # kx = 0: bit-exact integers
    assert np.all(kkz[F // 2] == F // 2)                                  # f = 0: sign(0) = 0


def test_gamma_from_the_plane_wave_normals():
    ang = np.array([-10.0, -0.25, 0.0, 7.5])
    g = MG.gamma(R.pw_normals(ang))
    ref = np.sin(np.deg2rad(ang)) / (2 - np.cos(np.deg2rad(ang)))
    assert np.allclose(g, ref, rtol=1e-12, atol=0) and g[2] == 0


# ---------------------------------------------------------------------------------------------------------------- argument errors, warnings
def _system(seq=None, xdc=None, N=8, M=3):
    xdc = xdc or Transducer.linear(N, PITCH)
    seq = seq or Sequence("PW", R.pw_normals(ANG[:M]), C0)
    return UltrasoundSystem(xdc, seq, Scan.cartesian(np.linspace(-1e-3, 1e-3, 3), np.linspace(5e-3, 6e-3, 4)), fs=FS)


def test_bfmigration_argument_errors():
    us = _system()
    x = torch.zeros((16, 8, 3), dtype=torch.complex64)
    with pytest.raises(DasError, match="Interp option not recognized: spline"):
        us.bfMigration(ChannelData(x, 0.0, FS), interp="spline")
    with pytest.raises(DasError, match="rectifyt0"):
        us.bfMigration(ChannelData(x, np.array([0.0, 1e-7, 2e-7]).reshape(1, 1, 3), FS))
    for bad in ((0, 8), (16, -2), (16.5, 8), (16, 8, 4)):
        with pytest.raises(DasError, match="Nfft"):
            us.bfMigration(ChannelData(x, 0.0, FS), Nfft=bad)
    with pytest.raises(DasError, match="complex64"):
        us.bfMigration(ChannelData(x.to(torch.complex128), 0.0, FS))
    with pytest.raises(DasError, match="receives"):
        us.bfMigration(ChannelData(x[:, :5], 0.0, FS))
    with pytest.raises(DasError, match="transmits"):
        us.bfMigration(ChannelData(x[:, :, :2], 0.0, FS))
    with pytest.raises(DasError, match="bsize"):
        us.bfMigration(ChannelData(x, 0.0, FS), bsize=0)


def test_bfmigration_issues_the_two_reference_warnings():
    """they are issued before anything touches a device: the call then ends in an argument error here"""
    x = torch.zeros((16, 8, 3), dtype=torch.float32)
    foc = np.array([[0.0, 1e-3, 2e-3], [0.0, 0.0, 0.0], [20e-3, 20e-3, 20e-3]])
    with pytest.warns(UserWarning, match='Expected a Sequence of type "PW", but instead it was type "FC". Unexpected results may occur.'):
        with pytest.raises(DasError):
            _system(seq=Sequence("FC", foc, C0)).bfMigration(ChannelData(x, 0.0, FS))
    with pytest.warns(UserWarning, match='Expected a TransducerArray but the Transducer is a TransducerConvex". Unexpected results may occur.'):
        with pytest.raises(DasError):
            _system(xdc=Transducer.convex(8, 40e-3, 0.5)).bfMigration(ChannelData(x, 0.0, FS))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(DasError, match="complex64"):
            _system().bfMigration(ChannelData(x, 0.0, FS))


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_abi_symbol_and_descriptor():
    assert "qdas_migration" in _lib.SYMBOLS and hasattr(_lib.lib(), "qdas_migration")
    D = _lib.MigrationDesc
    assert C.sizeof(D) == 120                                 # 6 extents, 5 doubles, 4 ints, 2 pointers
    assert (D.F.offset, D.fs.offset, D.pitch.offset, D.flag.offset, D.device.offset, D.tau.offset, D.gamma.offset) == (32, 48, 80, 88, 100, 104, 112)
    assert "migration" in __import__("qups_amd").__all__ and callable(MG.migrate) and callable(MG.compose)


def _desc(**kw):
    d = _lib.MigrationDesc()
    d.T, d.N, d.M, d.frames, d.F, d.K = 64, 16, 3, 1, 64, 16
    d.fs, d.fmod, d.t0, d.c0, d.pitch = FS, 0.0, T0, C0, PITCH
    d.flag, d.keep_tx, d.jacobian, d.device = 2, 0, 1, -1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("kw,code,text", [
    (dict(flag=4), 1, "interpolator"), (dict(flag=7), 1, "interpolator"), (dict(keep_tx=2), 1, "keep_tx"), (dict(jacobian=-1), 1, "jacobian"),
    (dict(T=1 << 31), 2, "extent"), (dict(K=1 << 32), 2, "extent"), (dict(F=0), 1, "positive"), (dict(K=0), 1, "positive"),
    (dict(fs=0.0), 1, "fs"), (dict(c0=-1.0), 1, "c0"), (dict(pitch=float("nan")), 1, "pitch"), (dict(t0=float("inf")), 1, "t0"),
    (dict(F=34), 6, "in-LDS"), (dict(K=17), 6, "in-LDS"), (dict(F=8193), 6, "in-LDS"), (dict(K=1), 6, "in-LDS"), (dict(K=1024), 6, "K outside"),
    (dict(), 1, "null data pointer"),
])
def test_c_abi_rejects_bad_descriptors_before_any_launch(kw, code, text):
    L = _lib.lib()
    assert L.qdas_migration(C.byref(_desc(**kw)), None, None, None) == code
    assert text in L.qdas_last_error().decode()


def test_c_abi_null_descriptor_empty_problem_and_routing_code():
    L = _lib.lib()
    assert L.qdas_migration(None, None, None, None) == 1
    for kw in (dict(T=0), dict(N=0), dict(M=0), dict(frames=0)):
        assert L.qdas_migration(C.byref(_desc(**kw)), None, None, None) == 0        # nothing to do, no device needed
    assert _lib.QDAS_ENOTLDS == 6
    assert MG.takes(64, 16) and MG.takes(8192, 8) and MG.takes(77, 18) and not MG.takes(34, 12) and not MG.takes(64, 1)
