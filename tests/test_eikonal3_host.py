"""Host side of the 3-D eikonal feature (no device): the float64 oracle (tests/eikonal3_ref.py) pinned by facts that follow from the update rule -- among
them that heap fast marching with msfm3d's rule lands on the fixed point of the classical upwind update, which is what the device iterates --, argument
errors and their texts, the C ABI's symbols and validation, the header's words on stream and work space, ``Transducer.matrix`` and the dispatch in
``bfEikonal``."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import qups_amd
from qups_amd import ChannelData, DasError, Scan, Sequence, Transducer, UltrasoundSystem, _lib, msfm3d
from qups_amd import eikonal as E
from tests import eikonal3_ref as R3
from tests import eikonal_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-12
# heap solver against brute-force fixed point: both solve the same discrete system in fp64, only rounding separates them (the roots are well conditioned:
# the discriminants are >= s^2 where a root is accepted).  1e-11 of the largest cell travel time is two decades under the device tests' 1e-9.
AGREE = 1e-11


def _close(a, b):
    return np.all(np.abs(np.asarray(a) - np.asarray(b)) <= REL * np.maximum(np.abs(b), 1e-300))


# ---------------------------------------------------------------------------------------------------------------- the oracle
def _interface_and_slab(shape):
    c = np.full(shape, 1500.0)
    c[shape[0] // 2:] = 75.0                                          # 20 : 1
    c[:, :2, :] = 3000.0                                              # a fast slab
    return c


@pytest.mark.parametrize("kind,shape,src", [("random", (9, 8, 7), [[3.0], [4.0], [2.0]]),
                                            ("interface", (8, 7, 9), [[2.0], [5.0], [3.0]]),
                                            ("homogeneous", (7, 7, 7), [[4.0, 1.0], [4.0, 7.0], [4.0, 2.0]])])
def test_oracle_heap_solver_lands_on_the_fixed_point_of_the_classical_update(kind, shape, src):
    """msfm3d's rule is not monotone (a third finite neighbour can RAISE its value from the two-term root to min + s), so the device iterates the classical
    upwind update instead; the heap solver, which keeps the minimum of the candidates a node receives while its neighbours freeze in ascending order, must
    produce that update's fixed point"""
    c = {"random": np.random.default_rng(1).uniform(1000.0, 2000.0, shape), "interface": _interface_and_slab(shape), "homogeneous": np.full(shape, 1500.0)}[kind]
    dp = 1e-4
    A = R3.fmm3(c, dp, src)
    B, sweeps = R3.fixed_point(c, dp, src)
    cell = dp / c.min()
    print(f"{kind}: max |heap - fixed point| = {np.abs(A - B).max() / cell:.3e} of the largest cell time, {sweeps} sweeps")
    assert np.isfinite(A).all() and np.abs(A - B).max() <= AGREE * cell


def test_oracle_rule_is_not_monotone_and_the_classical_update_is():
    """s = 1, t = (0, 0.9): the two-term root is 0.9954.  A finite t_z = 1.0454 above it makes msfm3d's rule put all three into one quadratic, whose root
    0.994 lies below t_z, and fall back to min + s = 1.0 -- a LARGER value than with t_z absent.  The classical update ignores a t_z above the two-term
    root and is monotone in it"""
    s = 1.0
    two = R3._rule([0.0, 0.9, R3.INF], s)
    assert abs(two - 0.5 * (0.9 + np.sqrt(2 - 0.81))) < 1e-15
    assert R3._rule([0.0, 0.9, two + 0.05], s) == 1.0 != two       # the three-term root lies below t_z: min + s, not the two-term root
    cl = lambda tz: float(R3.classical_update(np.array(0.0), np.array(0.9), np.array(tz), s))
    assert cl(two + 0.05) == cl(np.inf) and abs(cl(np.inf) - two) < 1e-15
    vals = [cl(tz) for tz in np.linspace(0.0, 1.5, 301)]
    assert np.all(np.diff(vals) >= 0)                                # monotone in t_z


def test_oracle_homogeneous_axes_through_a_corner_source():
    """along the three grid lines through a source in a corner only one neighbour ever counts: T = n dp / c"""
    dp, c0 = 0.25e-3, 1540.0
    T = R3.fmm3(np.full((11, 9, 7), c0), dp, [[1.2], [1.0], [1.9]])          # floors to node (0, 0, 0)
    assert T[0, 0, 0] == 0.0
    assert _close(T[:, 0, 0], np.arange(11) * dp / c0) and _close(T[0, :, 0], np.arange(9) * dp / c0) and _close(T[0, 0, :], np.arange(7) * dp / c0)
    F, _ = R3.fixed_point(np.full((11, 9, 7), c0), dp, [[1.2], [1.0], [1.9]])
    assert _close(F[:, 0, 0], np.arange(11) * dp / c0)


def test_oracle_a_one_node_thick_volume_is_the_2d_oracle():
    c = R.smooth_random(17, 13, seed=4)
    src2 = np.array([[3.0, 15.5], [4.0, 11.2]])
    ref = R.fmm(c, 1e-4, src2)
    T = R3.fmm3(c[:, :, None], 1e-4, np.vstack([src2, [[1.0, 1.0]]]))
    assert T.shape == (17, 13, 1)
    assert np.abs(T[:, :, 0] - ref).max() <= AGREE * 1e-4 / c.min()


def test_oracle_sampler_nodes_outside_and_a_trilinear_field():
    rng = np.random.default_rng(0)
    for shape in ((6, 5, 4), (2, 5, 3), (3, 1, 4), (1, 1, 2), (4, 2, 2)):
        T = rng.uniform(1, 2, shape)
        g = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
        v = R3.sample3(T, np.stack([x.ravel() + 1.0 for x in g]))
        assert np.array_equal(v, T.ravel())                            # weights 0, 1, 0, 0 exactly: the node's value bit for bit
    T = rng.uniform(1, 2, (6, 5, 4))
    out = R3.sample3(T, np.array([[0.999, 6.001, 3.0, 3.0, 3.0, 3.0, np.nan], [3.0, 3.0, 0.5, 5.5, 2.0, 2.0, 2.0], [2.0, 2.0, 2.0, 2.0, 0.9, 4.1, 2.0]]))
    assert np.all(np.isnan(out))
    # cubic convolution reproduces a trilinear field exactly -- with Keys' ghost nodes in the border cells as well
    i, j, l = np.meshgrid(np.arange(6.0), np.arange(5.0), np.arange(4.0), indexing="ij")
    q = lambda u, v, w: 1 + 0.3 * u - 0.2 * v + 0.5 * w + 0.05 * u * v - 0.03 * v * w + 0.02 * u * w + 0.01 * u * v * w
    P = np.stack([rng.uniform(0, 5, 300), rng.uniform(0, 4, 300), rng.uniform(0, 3, 300)])
    assert np.allclose(R3.sample3(q(i, j, l), P + 1.0), q(*P), rtol=1e-12, atol=1e-12)
    # a one-plane volume is the 2-D sampler
    T2 = rng.uniform(1, 2, (7, 6))
    P2 = np.stack([rng.uniform(1, 7, 50), rng.uniform(1, 6, 50)])
    assert np.array_equal(R3.sample3(T2[:, :, None], np.vstack([P2, np.ones((1, 50))])), R.sample(T2, P2))


# ---------------------------------------------------------------------------------------------------------------- arguments (no device is touched)
def test_msfm3d_argument_errors_and_texts():
    F = np.ones((8, 6, 5))
    with pytest.raises(DasError, match="Source points must be >= 1 to be within the field."):
        msfm3d(F, np.array([[2.0], [2.0], [0.5]]))
    with pytest.raises(DasError, match="Source points must be <= 8 in dimension 1 to be in the field."):
        msfm3d(F, np.array([[8.5], [2.0], [2.0]]))
    with pytest.raises(DasError, match="Source points must be <= 6 in dimension 2 to be in the field."):
        msfm3d(F, np.array([[2.0, 3.0], [2.0, 6.25], [1.0, 1.0]]))
    with pytest.raises(DasError, match="Source points must be <= 5 in dimension 3 to be in the field."):
        msfm3d(F, np.array([[2.0], [2.0], [5.5]]))
    with pytest.raises(DasError, match="not built"):
        msfm3d(F, np.array([[2.0], [2.0], [2.0]]), True)
    with pytest.raises(DasError, match="not built"):
        msfm3d(F, np.array([[2.0], [2.0], [2.0]]), False, True)
    with pytest.raises(DasError, match="3 x K"):
        msfm3d(F, np.array([[2.0], [2.0]]))
    with pytest.raises(DasError, match="3-D"):
        msfm3d(np.ones((8, 6)), np.array([[2.0], [2.0], [1.0]]))
    for name in ("msfm3d", "eikonal3", "eikonal3_tables", "travel_time_tables3", "scan_grid3", "pass_cap3"):
        assert name in E.__all__ and callable(getattr(E, name))
    assert "msfm3d" in qups_amd.__all__


def _volume(nx=9, ny=7, nz=11, step=1e-4):
    return Scan.cartesian(np.arange(nx) * step - 4e-4, np.arange(nz) * step, np.arange(ny) * step - 3e-4)


def test_scan_grid3_and_grid_coordinates():
    cgrd = _volume()
    og, dp, dims, axes, size = E.scan_grid3(cgrd)
    assert np.allclose(og, [-4e-4, -3e-4, 0.0]) and np.isclose(dp, 1e-4, rtol=1e-12)
    assert dims == (0, 1, 2) and axes == (2, 0, 1) and size == (11, 9, 7)       # 'ZXY': z along dimension 0, x along 1, y along 2
    Pi = cgrd.positions().reshape(3, -1, order="F")
    g = E.grid_coordinates(Pi, og, dp, axes)                                    # every pixel of the scan maps onto its own node
    i, j, l = np.meshgrid(np.arange(11), np.arange(9), np.arange(7), indexing="ij")
    assert g.shape == (3, 11 * 9 * 7)
    assert all(np.array_equal(g[d], v.ravel(order="F") + 1.0) for d, v in enumerate((i, j, l)))
    xdc = Transducer.matrix((3, 2), 2e-4)
    ge = E.grid_coordinates(xdc.positions(), og, dp, axes)
    assert np.array_equal(ge[0], np.ones(6)) and np.allclose(ge[1], [3, 5, 7, 3, 5, 7]) and np.allclose(ge[2], [3, 3, 3, 5, 5, 5])


def test_scan_grid3_rejects_what_the_reference_rejects():
    with pytest.raises(DasError, match="The simulation scan must have equally sized steps in all non-singleton dimensions."):
        E.scan_grid3(Scan.cartesian(np.linspace(-1e-3, 1e-3, 5), np.linspace(0, 2e-3, 5), np.linspace(0, 1e-3, 5)))
    with pytest.raises(DasError, match="three non-singleton dimensions"):
        E.scan_grid3(Scan.cartesian(np.linspace(-1e-3, 1e-3, 5), np.linspace(0, 2e-3, 5)))
    bent = _volume()
    bent.pos = bent.pos.copy()
    bent.pos[0] += 0.1 * bent.pos[2]                                            # sheared: x depends on two array dimensions
    with pytest.raises(DasError, match="Cartesian"):
        E.scan_grid3(bent)


# ---------------------------------------------------------------------------------------------------------------- the C ABI (no device)
def test_abi_symbols_struct_early_outs_and_pass_cap():
    L = _lib.lib()
    for s in ("qdas_eikonal3", "qdas_eikonal3_tables", "qdas_eikonal3_work_bytes", "qdas_eikonal3_pass_cap"):
        assert hasattr(L, s) and s in _lib.SYMBOLS
    assert C.sizeof(_lib.Eikonal3Desc) == 5 * 8 + 8 + 8 + 4 * 4 + 8 + 8
    assert L.qdas_eikonal3_pass_cap(161, 161, 241) == 8 * (161 + 161 + 241) + 64 and E.pass_cap3(8, 8, 8) == 256
    d = _lib.Eikonal3Desc()
    d.C1, d.C2, d.C3, d.K, d.npts, d.dp, d.base, d.device = 4, 0, 5, 3, 3, 1.0, 1, -1
    n, p = C.c_uint64(7), C.c_uint32(7)
    assert L.qdas_eikonal3(C.byref(d), None, None, None, None, 0, C.byref(p)) == 0 and p.value == 0      # an empty grid launches nothing
    assert L.qdas_eikonal3_work_bytes(C.byref(d), C.byref(n)) == 0 and n.value == 0
    d.C2, d.K, d.npts = 5, 0, 0
    assert L.qdas_eikonal3(C.byref(d), None, None, None, None, 0, None) == 0                              # no sources neither
    assert L.qdas_eikonal3_tables(C.byref(d), None, None, None) == 0
    d.K, d.npts, d.I = 2, 2, 0
    assert L.qdas_eikonal3_tables(C.byref(d), None, None, None) == 0                                      # no pixels
    # unsupported sizes
    d.K, d.npts = 65536, 65536
    assert L.qdas_eikonal3(C.byref(d), None, None, None, None, 0, None) == _lib.QDAS_EUNSUPPORTED and b"65535 source sets" in L.qdas_last_error()
    d.K, d.npts, d.C1, d.C2, d.C3 = 1, 1, 8 * 256, 8 * 256, 8 * 256
    assert L.qdas_eikonal3_work_bytes(C.byref(d), C.byref(n)) == _lib.QDAS_EUNSUPPORTED and b"2^24" in L.qdas_last_error()
    d.C1, d.C2, d.C3, d.I = 4, 5, 5, 2 ** 32 - 255
    assert L.qdas_eikonal3_tables(C.byref(d), None, None, None) == _lib.QDAS_EUNSUPPORTED and b"2^32 - 256 pixels" in L.qdas_last_error()


def test_abi_every_invalid_argument_is_refused_on_the_host():
    L = _lib.lib()
    d = _lib.Eikonal3Desc()
    d.C1, d.C2, d.C3, d.K, d.npts, d.dp, d.base, d.device = 4, 5, 6, 2, 3, 1.0, 1, -1
    call = lambda c=None, src=None, T=None, work=None, nbytes=0: L.qdas_eikonal3(C.byref(d), c, src, T, work, nbytes, None)
    err = lambda: L.qdas_last_error().decode()
    assert L.qdas_eikonal3(None, None, None, None, None, 0, None) == 1 and "null descriptor" in err()
    assert call() == 1 and "npts == K" in err()
    d.npts, d.dp = 2, 0.0
    assert call() == 1 and "grid step" in err()
    d.dp = float("nan")
    assert call() == 1 and "grid step" in err()
    d.dp = 1.0
    assert call() == 1 and "null data pointer" in err()
    one = np.ones(4 * 5 * 6 * 2)
    buf = np.zeros(1 << 16, np.uint8)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    src = np.array([[1.0, 1.0, 1.0], [2.0, 5.0, 6.5]])                          # the second point: third coordinate 6.5 > C3 = 6
    assert call(ptr(one), ptr(src), ptr(one), None, 1 << 16) == 1 and "null data pointer" in err()          # the work space is a data pointer too
    assert call(ptr(one), ptr(src), ptr(one), ptr(buf), 1 << 16) == 1 and "outside the grid" in err()
    src[1, 2] = 6.0
    n = C.c_uint64()
    assert L.qdas_eikonal3_work_bytes(C.byref(d), C.byref(n)) == 0 and 0 < n.value <= 1 << 16
    assert call(ptr(one), ptr(src), ptr(one), ptr(buf), n.value - 1) == 1 and "work space is too small" in err()
    assert L.qdas_eikonal3_work_bytes(C.byref(d), None) == 1 and "null pointer" in err()
    begin = np.array([0, 2, 1], np.uint64)                                      # does not ascend
    d.set_begin = begin.ctypes.data_as(C.POINTER(C.c_uint64))
    assert call(ptr(one), ptr(src), ptr(one), ptr(buf), n.value) == 1 and "set_begin must ascend" in err()
    begin[:] = [0, 0, 2]
    assert call(ptr(one), ptr(src), ptr(one), ptr(buf), n.value) == 1 and "a source set is empty" in err()
    d.set_begin = None
    d.base = 2
    assert call() == 1 and "0- or 1-based" in err()
    assert L.qdas_eikonal3_tables(C.byref(d), None, None, None) == 1 and "0- or 1-based" in err()
    d.base, d.I = 1, 10
    assert L.qdas_eikonal3_tables(C.byref(d), None, None, None) == 1 and "null data pointer" in err()
    d.C2 = 0
    assert L.qdas_eikonal3_tables(C.byref(d), None, None, None) == 1 and "empty grid" in err()


def test_abi_work_bytes_grows_with_tiles_sets_and_points():
    L = _lib.lib()

    def nbytes(C1, C2, C3, K, npts=None):
        d = _lib.Eikonal3Desc()
        d.C1, d.C2, d.C3, d.K, d.npts, d.dp, d.base, d.device = C1, C2, C3, K, K if npts is None else npts, 1.0, 1, -1
        begin = np.zeros(K + 1, np.uint64)
        begin[1:] = np.arange(1, K + 1) + (d.npts - K)
        d.set_begin = begin.ctypes.data_as(C.POINTER(C.c_uint64))
        n = C.c_uint64()
        assert L.qdas_eikonal3_work_bytes(C.byref(d), C.byref(n)) == 0
        return n.value

    pairs = lambda C1, C2, C3, K: K * -(-C1 // 8) * -(-C2 // 8) * -(-C3 // 8)
    for shape in ((8, 8, 8, 1), (161, 161, 241, 16), (17, 5, 9, 5)):
        n = nbytes(*shape)
        assert n % 256 == 0 and n >= pairs(*shape) * (2 * 4 + 2 * 8) + 16 * shape[3]      # two flag arrays, two lists, the points
        assert n <= pairs(*shape) * 24 + 16 * shape[3] + 5 * 256                            # ... and nothing that grows with the nodes
    assert nbytes(8, 8, 8, 1) == nbytes(7, 3, 1, 1) < nbytes(64, 64, 8, 1) < nbytes(65, 64, 8, 1)          # (every part is rounded up to 256 bytes)
    assert nbytes(24, 24, 24, 3, npts=3000) > nbytes(24, 24, 24, 3)


def test_header_carries_the_stream_in_the_descriptor_and_documents_the_work_space():
    hdr = open(os.path.join(ROOT, "include", "qdas.h")).read()
    protos = re.findall(r"^(?:int|uint32_t) qdas_eikonal3\w*\([^;]*\);", hdr, re.M | re.S)
    assert len(protos) == 4 and not any("stream" in p for p in protos)
    a = hdr.index("eikonal3.hip")
    doc = hdr[a:hdr.index("} qdas_eikonal3_desc;")]
    assert "void    *queue;" in doc and "WAITS" in doc and "WORK SPACE" in doc and "nothing the work space held before the call is read" in doc
    assert "qdas_eikonal3_work_bytes" in doc and "QDAS_ENOCONV" in doc
    assert _lib.lib().qdas_version() == 103


# ---------------------------------------------------------------------------------------------------------------- Transducer.matrix
def test_transducer_matrix_positions_follow_the_reference_formula():
    """src/TransducerMatrix.m:130-138: linspace(-w/2, w/2, numd(1)) by linspace(-h/2, h/2, numd(end)), ndgrid order (x fastest), z = 0"""
    xdc = Transducer.matrix((4, 3), (0.3e-3, 0.5e-3), fc=3e6, offset=(1e-3, -2e-3, 0.5e-3))
    p = xdc.positions()
    assert p.shape == (3, 12) and xdc.numel == 12 and xdc.fc == 3e6 and xdc.kind == "TransducerMatrix"
    x, y = np.linspace(-0.45e-3, 0.45e-3, 4), np.linspace(-0.5e-3, 0.5e-3, 3)
    for iy in range(3):
        for ix in range(4):
            assert np.allclose(p[:, ix + 4 * iy], [x[ix] + 1e-3, y[iy] - 2e-3, 0.5e-3], rtol=0, atol=1e-18)
    assert np.array_equal(xdc.normals, np.tile([[0.0], [0.0], [1.0]], (1, 12)))
    sq = Transducer.matrix(3, 0.2e-3)
    assert sq.numel == 9 and np.allclose(sq.positions()[:, 0], [-0.2e-3, -0.2e-3, 0]) and np.allclose(sq.positions()[:, 5], [0.2e-3, 0.0, 0.0])


# ---------------------------------------------------------------------------------------------------------------- bfEikonal's dispatch
class _Reached(Exception):
    pass


def test_bfEikonal_chooses_the_path_before_it_reads_the_grid(monkeypatch):
    """a grid with two non-singleton dimensions still reaches scan_grid, one with three reaches scan_grid3 -- and neither touches a device before"""
    def stop(name):
        def f(scan):
            raise _Reached(name)
        return f
    monkeypatch.setattr(E, "scan_grid", stop("2"))
    monkeypatch.setattr(E, "scan_grid3", stop("3"))
    flat = Scan.cartesian(np.linspace(-2e-3, 2e-3, 41), np.linspace(0, 5e-3, 51))
    us = UltrasoundSystem(Transducer.matrix(2, 0.3e-3), Sequence("FSA", c0=1500.0), flat)
    chd = ChannelData(np.zeros((16, 4, 4), np.complex64), 0.0, 20e6)
    with pytest.raises(_Reached, match="2"):
        us.bfEikonal(chd, 1500.0)
    with pytest.raises(_Reached, match="2"):
        us.bfEikonal(chd, 1500.0, Scan.cartesian([0.0], np.linspace(0, 5e-3, 51), np.linspace(0, 5e-3, 51)))
    with pytest.raises(_Reached, match="2"):
        us.bfEikonal(chd, 1500.0, Scan.cartesian([0.0], np.linspace(0, 5e-3, 51)))          # a line: scan_grid's own refusal follows
    with pytest.raises(_Reached, match="3"):
        us.bfEikonal(chd, 1500.0, _volume())
    monkeypatch.undo()
    with pytest.raises(DasError, match="equally sized steps"):
        us.bfEikonal(chd, 1500.0, Scan.cartesian(np.linspace(-1e-3, 1e-3, 5), np.linspace(0, 2e-3, 5), np.linspace(0, 1e-3, 5)))
    with pytest.raises(DasError, match="array of the grid's size"):
        us.bfEikonal(chd, np.full((5, 5, 5), 1500.0), _volume())
