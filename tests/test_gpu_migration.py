"""``qdas_migration`` (csrc/migration.hip), ``qups_amd.migration.compose`` and ``UltrasoundSystem.bfMigration`` on the device against the float64
restatement (tests/migration_ref.py) on identical complex64 random data.  Metric: ``max|b - ref| / max|ref|``.

Shapes are chosen to break staging, not to resemble a workload: native, padded and truncated lengths, radices 2 / 3 / 5 / 7 / 11, the 512-thread
stage path (F = 8192), a length the kernels do not take (34 = 2 x 17: routed to ``compose``, asserted through the library's return code).

Bounds.  Largest error measured on an MI355X over every fused case of this file: 4.2e-7 (the 8192-point case; 2.1e-7 to 3.5e-7 elsewhere); over every
``compose`` case: 1.7e-6.  So the bounds are 4.2e-6 and 1.7e-5.
The bound is ten times the measured value and never above the project's fp32 bound of 1e-4: it exists to catch indexing, shift
and padding errors, which are O(1).  ``compose`` hands ``wsinterpd`` fp32 sample indices and is the less accurate of the two."""
import functools

import numpy as np
import pytest
import torch

from qups_amd import ChannelData, Scan, Sequence, Transducer, UltrasoundSystem, _lib
from qups_amd import migration as MG
from tests import migration_ref as R

pytestmark = pytest.mark.gpu

FS, C0, PITCH, T0 = 20e6, 1540.0, 0.3e-3, 1.3e-6
MEASURED_FUSED, MEASURED_COMPOSE = 4.2e-7, 1.7e-6
BOUND_FUSED, BOUND_COMPOSE = min(10 * MEASURED_FUSED, 1e-4), min(10 * MEASURED_COMPOSE, 1e-4)
ANGLES = (-3.0, 0.0, 5.0, 2.0, -6.0)

#        T     N   M  Nfft          what
SHAPES = [
    (64, 16, 3, None),            # native, 2^6 x 2^4
    (48, 12, 3, (96, 24)),        # padded, 2^5 3 x 2^3 3
    (60, 20, 1, (60, 20)),        # 3 4 5 x 4 5
    (77, 18, 2, (77, 18)),        # 7 11 x 2 9
    (80, 20, 3, (64, 16)),        # both truncated
    (100, 40, 2, (770, 77)),      # 11 7 5 2, the 512-thread variant below 8192 points x 11 7
    (120, 50, 1, (1287, 91)),     # 13 11 9 x 13 7
]
BIG = (8192, 8, 1, (8192, 8))     # the 512-thread stage path
ODD = (34, 12, 2, (34, 12))       # 17 is no radix: compose
INTERPS = ("nearest", "linear", "cubic", "cubic_dev", "lanczos3")


def _fk(shape):
    T, N, _, nfft = shape
    return (T, N) if nfft is None else nfft


@pytest.fixture(scope="module", autouse=True)
def margins():
    """float64, CPU: every kkz of a tested shape lies at least 1e-4 sample from each discontinuity of its interpolator (the exact kx = 0 column and
    f = 0 row are the only points left out) -- at least 6x the fp32 index spacing at F <= 128, which is what ``compose`` needs.  The 8192-point case
    is compared for the fused path only (fp64 indices), with ``linear``."""
    for shape in SHAPES + [ODD]:
        for interp in (INTERPS if shape is SHAPES[0] else ("cubic",)):
            m = R.discontinuity_margin(*_fk(shape), FS, PITCH, C0, interp)
            assert m >= 1e-4, (shape, interp, m)
    assert R.discontinuity_margin(*_fk(BIG), FS, PITCH, C0, "linear") >= 1e-4


@functools.lru_cache(maxsize=None)
def _data(T, N, M, frames=1, seed=0):
    rng = np.random.default_rng(seed + 1000 * T + N)
    x = (rng.standard_normal((T, N, M, frames)) + 1j * rng.standard_normal((T, N, M, frames))).astype(np.complex64)
    elem = np.stack([(np.arange(N) - (N - 1) / 2) * PITCH, np.zeros(N), np.zeros(N)])
    ang = ANGLES[:M] if M <= len(ANGLES) else tuple(np.linspace(-6, 6, M))
    return x, R.pw_delays(elem, ang, C0), R.gamma(ang)


@functools.lru_cache(maxsize=None)
def _ref(T, N, M, nfft, interp="cubic", jacobian=True, keep_tx=False, fmod=0.0, frames=1):
    x, tau, gam = _data(T, N, M, frames)
    return R.migrate(x, T0, FS, tau, gam, PITCH, C0, nfft, fmod, interp, jacobian, keep_tx)


def _err(b, ref, what):
    b = b.cpu().numpy()
    assert b.shape == ref.shape and b.dtype == np.complex64, (b.shape, ref.shape, b.dtype)
    e = float(np.abs(b - ref).max() / np.abs(ref).max())
    print(f"migration {what}: rel_err={e:.3e}")
    return e


def _run(fn, shape, interp="cubic", jacobian=True, keep_tx=False, fmod=0.0, frames=1, **kw):
    T, N, M, nfft = shape
    x, tau, gam = _data(T, N, M, frames)
    b = fn(torch.from_numpy(x).cuda(), T0, FS, tau, gam, PITCH, C0, nfft, fmod, interp, jacobian, keep_tx, **kw)
    torch.cuda.synchronize()
    return _err(b, _ref(T, N, M, nfft, interp, jacobian, keep_tx, fmod, frames), f"{fn.__name__} {shape} {interp} jac={jacobian} keep_tx={keep_tx} fmod={fmod} frames={frames}")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}-{s[3]}")
def test_fused_shapes(shape):
    assert MG.takes(*_fk(shape))
    assert _run(MG.migrate, shape) <= BOUND_FUSED


def test_fused_8192_points_linear():
    assert MG.takes(*_fk(BIG))
    assert _run(MG.migrate, BIG, "linear") <= BOUND_FUSED


@pytest.mark.parametrize("interp", INTERPS)
def test_fused_interpolators(interp):
    assert _run(MG.migrate, SHAPES[0], interp) <= BOUND_FUSED


@pytest.mark.parametrize("kw", [dict(keep_tx=True), dict(jacobian=False), dict(fmod=2.5e6), dict(frames=2), dict(frames=2, keep_tx=True)],
                         ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
def test_fused_options(kw):
    assert _run(MG.migrate, SHAPES[1], **kw) <= BOUND_FUSED


def test_fused_noncontiguous_view():
    T, N, M, nfft = SHAPES[0]
    x, tau, gam = _data(T, N, M)
    big = torch.zeros((2 * T, N + 3, M, 1), dtype=torch.complex64, device="cuda")
    big[::2, 1:N + 1] = torch.from_numpy(x).cuda()
    view = big[::2, 1:N + 1]
    assert not view.is_contiguous()
    assert _err(MG.migrate(view, T0, FS, tau, gam, PITCH, C0), _ref(T, N, M, nfft), "view") <= BOUND_FUSED


@pytest.mark.parametrize("per_block,fill", [(2, 1), (4, None), (4, 32), (1, None)])
def test_fused_transmit_blocks_and_slices(per_block, fill, monkeypatch):
    """five transmits: one past a block of four (and of two twice), the block's transmits in one slice, one slice each, and slices of two"""
    shape = (64, 16, 5, None)
    monkeypatch.setenv("QDAS_MIGRATION_BLOCK_BYTES", str(per_block * 64 * 16 * 8))
    if fill is not None:
        monkeypatch.setenv("QDAS_MIGRATION_FILL", str(fill))
    assert _run(MG.migrate, shape) <= BOUND_FUSED
    assert _run(MG.migrate, shape, keep_tx=True) <= BOUND_FUSED


def test_results_are_bit_reproducible():
    T, N, M, nfft = SHAPES[1]
    x, tau, gam = _data(T, N, M)
    xd = torch.from_numpy(x).cuda()
    a = MG.migrate(xd, T0, FS, tau, gam, PITCH, C0, nfft)
    b = MG.migrate(xd, T0, FS, tau, gam, PITCH, C0, nfft)
    assert torch.equal(a, b)


def test_length_with_radix_17_is_routed_to_compose():
    T, N, M, nfft = ODD
    x, tau, gam = _data(T, N, M)
    xd = torch.from_numpy(x).cuda()
    with pytest.raises(_lib.QdasError) as e:
        MG.migrate(xd, T0, FS, tau, gam, PITCH, C0, nfft)
    assert e.value.code == _lib.QDAS_ENOTLDS and not MG.takes(*nfft)
    ref = _ref(T, N, M, nfft)
    assert _err(MG.bmode(xd, T0, FS, tau, gam, PITCH, C0, nfft), ref, "bmode 34x12") <= BOUND_COMPOSE
    assert _err(MG.compose(xd, T0, FS, tau, gam, PITCH, C0, nfft), ref, "compose 34x12") <= BOUND_COMPOSE


@pytest.mark.parametrize("shape", SHAPES[:4], ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_compose_shapes(shape):
    assert _run(MG.compose, shape) <= BOUND_COMPOSE
    if shape[2] > 1:
        assert _run(MG.compose, shape, keep_tx=True, bsize=2) <= BOUND_COMPOSE


def _psf_system():
    N, T = 32, 512
    xdc = Transducer.linear(N, PITCH)
    ang = (-5.0, 0.0, 5.0)
    us = UltrasoundSystem(xdc, Sequence("PW", R.pw_normals(ang), C0), Scan.cartesian(np.linspace(-4e-3, 4e-3, 5), np.linspace(10e-3, 20e-3, 5)), fs=FS)
    scat = np.array([2e-3, 0.0, 15e-3])
    t0 = 12e-6
    x = R.gaussian_echoes(T, xdc.positions(), ang, scat, t0, FS, C0)
    return us, ChannelData(torch.from_numpy(x.astype(np.complex64)), t0, FS), scat, ang


def test_psf_through_bfmigration():
    """reference test/BFTest.m:306-316: Nfft = [2T, 4N], the image is non-zero and its peak lies within 1.1 mm of the scatterer; against the restatement too"""
    us, chd, scat, ang = _psf_system()
    T, N = chd.data.shape[:2]
    b, bscan = us.bfMigration(chd, (2 * T, 4 * N))
    torch.cuda.synchronize()
    assert tuple(b.shape) == (T, N) and b.dtype == torch.complex64 and bscan.size == (T, N, 1)
    mag = b.abs().cpu().numpy()
    assert mag.max() > 0
    iz, ix = np.unravel_index(np.argmax(mag), mag.shape)
    P = bscan.positions()[:, iz, ix, 0]
    assert np.hypot(P[0] - scat[0], P[2] - scat[2]) <= 1.1e-3, (P, scat)
    tau = R.pw_delays(us.xdc.positions(), ang, C0)
    ref = R.migrate(chd.data.numpy(), chd.t0, FS, tau, R.gamma(ang), PITCH, C0, (2 * T, 4 * N))
    assert _err(b, ref, "psf") <= BOUND_FUSED

