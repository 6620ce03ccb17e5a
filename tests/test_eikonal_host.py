"""Host side of the eikonal feature (no device): the float64 oracle (tests/eikonal_ref.py) pinned by facts that follow from the update rule,
argument errors and their texts, the grid-coordinate mapping, the transmit-reuse decision, the C ABI's symbols and validation."""
import ctypes as C
import os

import numpy as np
import pytest

from qups_amd import DasError, Scan, Sequence, Transducer, UltrasoundSystem, _lib, msfm
from qups_amd import eikonal as E
from tests import eikonal_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-12


def _close(a, b):
    return np.all(np.abs(np.asarray(a) - np.asarray(b)) <= REL * np.maximum(np.abs(b), 1e-300))


# ---------------------------------------------------------------------------------------------------------------- the oracle
def test_oracle_homogeneous_axes_through_an_edge_source():
    """along the grid row and column through a source on the edge only one neighbour ever counts: T = k dp / c"""
    dp, c0 = 0.25e-3, 1540.0
    T = R.fmm(np.full((31, 23), c0), dp, [[1.0], [9.3]])             # node (0, 8), on the edge i = 0
    assert T[0, 8] == 0.0
    assert _close(T[:, 8], np.arange(31) * dp / c0)
    assert _close(T[0, :], np.abs(np.arange(23) - 8) * dp / c0)


def test_oracle_layers_down_the_source_column():
    """laterally uniform layers: down the column under the source T = sum of dp / c_k"""
    dp = 0.2e-3
    cz = np.repeat([1400.0, 1600.0, 1500.0, 1450.0], 10)
    c = np.repeat(cz[:, None], 27, axis=1)
    T = R.fmm(c, dp, [[1.0], [14.0]])
    assert _close(T[1:, 13], np.cumsum(dp / cz[1:]))


def test_oracle_symmetry_about_the_source_column():
    c = R.layers_disc(41, 33)
    c = 0.5 * (c + c[:, ::-1])
    T = R.fmm(c, 1e-4, [[5.0], [17.0]])                              # the middle column of 33
    assert _close(T, T[:, ::-1])


def test_oracle_multi_point_source_is_the_minimum_of_single_sources():
    c = R.smooth_random(25, 19, seed=3)
    a, b = R.fmm(c, 1e-4, [[3.0], [4.0]]), R.fmm(c, 1e-4, [[20.0], [15.0]])
    both = R.fmm(c, 1e-4, [[3.0, 20.0], [4.0, 15.0]])
    assert both[2, 3] == 0 and both[19, 14] == 0
    assert np.all(both <= np.minimum(a, b) * (1 + 1e-12))


def test_oracle_sampler_node_centred_pixels_and_outside():
    rng = np.random.default_rng(0)
    for shape in ((9, 7), (2, 5), (3, 1), (1, 4)):
        T = rng.uniform(1, 2, shape)
        i, j = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
        v = R.sample(T, np.stack([i.ravel() + 1.0, j.ravel() + 1.0]))
        assert np.array_equal(v, T.ravel())                            # weights 0, 1, 0, 0 exactly
    T = rng.uniform(1, 2, (9, 7))
    out = R.sample(T, np.array([[0.999, 9.001, 5.0, 5.0, np.nan], [3.0, 3.0, 0.5, 7.5, 2.0]]))
    assert np.all(np.isnan(out))
    # cubic convolution with Keys' ghost nodes reproduces a quadratic exactly, border cells included
    i, j = np.meshgrid(np.arange(9.0), np.arange(7.0), indexing="ij")
    q = lambda u, v: 1 + 0.3 * u - 0.2 * v + 0.05 * u * u + 0.02 * v * v + 0.01 * u * v
    P = np.stack([rng.uniform(0, 8, 200), rng.uniform(0, 6, 200)])
    assert np.allclose(R.sample(q(i, j), P + 1.0), q(P[0], P[1]), rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------- arguments (no device is touched)
def test_msfm_argument_errors_and_texts():
    F = np.ones((8, 6))
    with pytest.raises(DasError, match="Source points must be >= 1 to be within the field."):
        msfm(F, np.array([[0.5], [2.0]]))
    with pytest.raises(DasError, match="Source points must be <= 8 in dimension 1 to be in the field."):
        msfm(F, np.array([[8.5], [2.0]]))
    with pytest.raises(DasError, match="Source points must be <= 6 in dimension 2 to be in the field."):
        msfm(F, np.array([[2.0, 3.0], [2.0, 6.25]]))
    with pytest.raises(DasError, match="not built"):
        msfm(F, np.array([[2.0], [2.0]]), True)
    with pytest.raises(DasError, match="not built"):
        msfm(F, np.array([[2.0], [2.0]]), False, True)
    with pytest.raises(DasError, match="3-D"):
        msfm(np.ones((4, 4, 4)), np.array([[2.0], [2.0], [2.0]]))


def _system(nel=4, rx=None, x=None, z=None):
    xdc = Transducer.linear(nel, 0.3e-3)
    scan = Scan.cartesian(np.linspace(-2e-3, 2e-3, 41) if x is None else x, np.linspace(0, 5e-3, 51) if z is None else z)
    return UltrasoundSystem(xdc, Sequence("FSA", c0=1500.0), scan, rx=rx)


def test_scan_grid_and_grid_coordinates():
    us = _system()
    og, dp, dims, axes, size = E.scan_grid(us.scan)
    assert np.allclose(og, [-2e-3, 0, 0]) and np.isclose(dp, 1e-4, rtol=1e-12)
    assert dims == (0, 1) and axes == (2, 0) and size == (51, 41)           # 'ZXY': z along dimension 0, x along dimension 1
    g = E.grid_coordinates(us.rx.positions(), og, dp, axes)                 # (P - origin) / dp + 1, z first
    assert g.shape == (2, 4)
    assert np.array_equal(g[0], np.ones(4))                                 # the elements lie on z = 0: the first node, exactly
    assert np.allclose(g[1], (us.rx.positions()[0] + 2e-3) / 1e-4 + 1, rtol=0, atol=1e-9)
    assert np.array_equal(np.floor(g[1]), [16, 19, 22, 25])                 # (what msfm floors them to)
    # every pixel of the scan maps onto its own node
    Pi = us.scan.positions().reshape(3, -1, order="F")
    gi = E.grid_coordinates(Pi, og, dp, axes)
    i, j = np.meshgrid(np.arange(51), np.arange(41), indexing="ij")
    assert np.array_equal(gi[0], i.ravel(order="F") + 1.0) and np.array_equal(gi[1], j.ravel(order="F") + 1.0)


def test_scan_grid_rejects_what_the_reference_rejects():
    with pytest.raises(DasError, match="The simulation scan must have equally sized steps in all non-singleton dimensions."):
        E.scan_grid(Scan.cartesian(np.linspace(-2e-3, 2e-3, 41), np.linspace(0, 5e-3, 41)))
    with pytest.raises(DasError, match="one singleton dimension"):
        E.scan_grid(Scan.cartesian(np.linspace(-1e-3, 1e-3, 5), np.linspace(0, 2e-3, 5), np.linspace(0, 2e-3, 5)))
    with pytest.raises(DasError, match="one singleton dimension"):
        E.scan_grid(Scan.cartesian([0.0], np.linspace(0, 2e-3, 5)))
    with pytest.raises(DasError, match="Cartesian"):
        E.scan_grid(Scan.polar(np.linspace(1e-3, 2e-3, 5), np.linspace(-10, 10, 5)))


def test_transmit_reuse_decision():
    assert E.same_aperture(_system())                                        # tx is rx
    assert E.same_aperture(_system(rx=Transducer.linear(4, 0.3e-3)))         # another object, equal positions
    assert not E.same_aperture(_system(rx=Transducer.linear(4, 0.2e-3)))
    assert not E.same_aperture(_system(rx=Transducer.linear(6, 0.3e-3)))


def test_bfEikonal_argument_errors_come_before_any_device_work():
    from qups_amd import ChannelData
    us = _system()
    bad_m = ChannelData(np.zeros((16, 4, 3), np.complex64), 0.0, 20e6)
    with pytest.raises(DasError, match="Number of transmits must match number of transmitter elements."):
        us.bfEikonal(bad_m, 1500.0)
    bad_n = ChannelData(np.zeros((16, 5, 4), np.complex64), 0.0, 20e6)
    with pytest.raises(DasError, match="Number of receives must match number of receiver elements."):
        us.bfEikonal(bad_n, 1500.0)
    ok = ChannelData(np.zeros((16, 4, 4), np.complex64), 0.0, 20e6)
    with pytest.raises(DasError, match="equally sized steps"):
        us.bfEikonal(ok, 1500.0, Scan.cartesian(np.linspace(-2e-3, 2e-3, 41), np.linspace(0, 5e-3, 41)))
    with pytest.raises(DasError, match="array of the grid's size"):
        us.bfEikonal(ok, np.full((5, 5), 1500.0))


# ---------------------------------------------------------------------------------------------------------------- the C ABI (no device)
def test_abi_symbols_struct_and_validation():
    L = _lib.lib()
    for s in ("qdas_eikonal", "qdas_eikonal_tables", "qdas_eikonal_last_passes", "qdas_eikonal_pass_cap"):
        assert hasattr(L, s) and s in _lib.SYMBOLS
    assert C.sizeof(_lib.EikonalDesc) == 5 * 8 + 8 + 4 * 4 + 8
    assert L.qdas_eikonal_pass_cap(481, 321) == 8 * (481 + 321) + 64 and E.pass_cap(16, 16) == 320
    d = _lib.EikonalDesc()
    d.C1, d.C2, d.K, d.npts, d.dp, d.base = 0, 5, 3, 3, 1.0, 1
    assert L.qdas_eikonal(C.byref(d), None, None, None, None) == 0              # an empty grid launches nothing
    d.C1, d.K, d.npts = 5, 0, 0
    assert L.qdas_eikonal(C.byref(d), None, None, None, None) == 0              # no sources neither
    assert L.qdas_eikonal_tables(C.byref(d), None, None, None, None) == 0
    d.K, d.npts = 2, 3
    assert L.qdas_eikonal(C.byref(d), None, None, None, None) == 1 and b"npts == K" in L.qdas_last_error()
    d.npts, d.dp = 2, 0.0
    assert L.qdas_eikonal(C.byref(d), None, None, None, None) == 1 and b"grid step" in L.qdas_last_error()
    d.dp = 1.0
    assert L.qdas_eikonal(C.byref(d), None, None, None, None) == 1 and b"null data pointer" in L.qdas_last_error()
    src = np.array([[1.0, 1.0], [6.5, 2.0]])                                     # the second point: first coordinate 6.5 > C1 = 5
    one = np.ones(25)
    assert L.qdas_eikonal(C.byref(d), C.c_void_p(one.ctypes.data), C.c_void_p(src.ctypes.data), C.c_void_p(one.ctypes.data), None) == 1
    assert b"outside the grid" in L.qdas_last_error()
    d.base = 2
    assert L.qdas_eikonal(C.byref(d), None, None, None, None) == 1 and b"0- or 1-based" in L.qdas_last_error()
    hdr = open(os.path.join(ROOT, "include", "qdas.h")).read()
    assert "QDAS_ENOCONV" in hdr and _lib.QDAS_ENOCONV == 5
