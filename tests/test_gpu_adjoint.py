"""``UltrasoundSystem.bfAdjoint`` / ``qdas_adjoint`` on the device against the float64 restatement (tests/adjoint_ref.py) on identical complex64 data,
fp32 positions and fp32 reciprocal sound speeds.  The shapes are chosen to break tiling (pixel tiles of 128 = 4 x 32, aperture chunks of 32, transmit
tiles of 32 in groups of 1 or 2), not to look like a workload.

Metric: ``max|b - b_ref| / max|b_ref|``.  The project's fp32 bound is 1e-4; with K <= 128 the phase error is far inside it -- the bound is
there to catch indexing and padding errors, which are O(1).  When the bound was set the largest value measured over this file on an MI355X was 3.6e-7
(I = 1, N = V = 1), more than 10 x under that bound, so the bound used here is 10 x that value: 3.6e-6.  (Cases added since measure up to 3.9e-7.)"""
import numpy as np
import pytest
import torch

from qups_amd import ChannelData, DasError, Scan, Sequence, Transducer, UltrasoundSystem
from qups_amd import adjoint as A
from tests import adjoint_ref as R

pytestmark = pytest.mark.gpu

TOL = 3.6e-6
FS, C0 = 20e6, 1540.0


def _system(kind, N, V, nz, nx, seed=0):
    xdc = Transducer.linear(N, 0.3e-3)
    if kind == "FSA":
        seq = Sequence("FSA", None, C0, N)
    elif kind == "PW":
        th = np.deg2rad(np.linspace(-10, 10, V)) if V > 1 else np.array([np.deg2rad(3.0)])
        seq = Sequence("PW", np.stack([np.sin(th), 0 * th, np.cos(th)]), C0, V)
    else:                                                   # FC
        seq = Sequence("FC", np.stack([np.linspace(-1e-3, 1e-3, V), np.zeros(V), np.linspace(8e-3, 11e-3, V)]), C0, V)
    x = np.linspace(-1.1e-3, 1.3e-3, nx) if nx > 1 else np.array([0.2e-3])
    z = np.linspace(6e-3, 12e-3, nz) if nz > 1 else np.array([9e-3])
    return UltrasoundSystem(xdc, seq, Scan.cartesian(x, z), fs=FS)


def _data(T, N, V, F=(), seed=0):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((T, N, V) + F) + 1j * rng.standard_normal((T, N, V) + F)).astype(np.complex64)
    t0 = 4e-6 + rng.uniform(0, 1e-6, V) if V > 1 else 4e-6
    return x, t0


def _pulse_data(T, N, V, seed=0):
    """band-limited: a Gaussian pulse at 5 MHz with a random delay per trace"""
    rng = np.random.default_rng(seed)
    t = np.arange(T)[:, None, None] / FS
    d = rng.uniform(1.0e-6, 3.0e-6, (1, N, V))
    x = np.exp(-0.5 * ((t - d) / 0.15e-6) ** 2) * np.exp(2j * np.pi * 5e6 * (t - d))
    return x.astype(np.complex64), 4e-6


def _oracle(us, x, t0, fmod=0.0, fthresh=-np.inf, Nfft=None, c0=C0, a_n=None, a_m=None, a_mn=None, keep_tx=False, keep_rx=False):
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    I = int(np.prod(us.scan.size))
    Pi = f32(np.asarray(us.scan.positions()).reshape((3, I), order="F"))
    cinv = f32(1.0 / np.asarray(c0, float).reshape(-1, order="F"))
    off = R.t0_offset(us.seq.type, us.seq.focus, us.seq.c0)
    tau_foc = np.asarray(us.seq.delays(us.tx), float) + off.reshape(1, -1)
    apod_tx = f32(us.seq.apodization(us.tx))
    X = R.spectrum(x, t0, FS, fmod, Nfft, off)
    bins = R.select_bins(X, FS, fthresh)
    col = lambda a, n: None if a is None else f32(np.broadcast_to(a, us.scan.size + (n,)).reshape((I, n), order="F"))
    b = R.adjoint(X, bins, FS, Pi, f32(us.rx.positions()), f32(us.tx.positions()), np.broadcast_to(cinv, (I,)), tau_foc, apod_tx,
                  col(a_n, x.shape[1]), col(a_m, x.shape[2]), None if a_mn is None else f32(a_mn), keep_tx=keep_tx, keep_rx=keep_rx)
    return b, bins


def _err(b, ref, what):
    b = b.cpu().numpy().astype(np.complex128)
    b = b.reshape(ref.shape, order="F") if b.size == ref.size else b
    e = np.abs(b - ref).max() / np.abs(ref).max()
    print(f"adjoint {what}: rel err {e:.3e} (bound {TOL:g})")
    return e


def _run(us, x, t0, **kw):
    return us.bfAdjoint(ChannelData(torch.from_numpy(x).cuda(), t0, FS), **kw)


def _flat(b, us):
    """I1 x I2 x I3 x N' x V' -> the oracle's I x [N] x [V] (kept dimensions only), column-major pixels"""
    I = int(np.prod(us.scan.size))
    a = b.cpu().numpy().reshape((I,) + tuple(b.shape[3:]), order="F")
    return a.reshape([I] + [n for n in a.shape[1:] if n > 1] if a.ndim > 1 else [I])


@pytest.fixture(scope="module")
def core():
    us = _system("PW", 20, 7, 37, 5)
    x, t0 = _data(96, 20, 7, seed=1)
    ref, bins = _oracle(us, x, t0, fmod=2.5e6)
    return us, x, t0, ref, bins


def test_core_parity_pw(core):
    us, x, t0, ref, bins = core
    assert us.scan.size == (37, 5, 1) and len(bins) == 48
    b, used = _run(us, x, t0, fmod=2.5e6, return_bins=True)
    assert tuple(b.shape) == (37, 5, 1, 1, 1) and b.dtype == torch.complex64
    assert np.array_equal(used, bins)
    assert _err(torch.from_numpy(_flat(b, us)), ref, "core PW 37x5, N=20, V=7") <= TOL


def test_fsa_one_past_an_mfma_edge():
    us = _system("FSA", 33, 33, 64, 3)
    x, t0 = _data(64, 33, 33, seed=2)
    ref, _ = _oracle(us, x, t0)
    assert _err(torch.from_numpy(_flat(_run(us, x, t0), us)), ref, "FSA N=M=V=33, I=64x3") <= TOL


def test_more_than_one_transmit_group():
    """V = 70: two groups of 64 transmits, the second with 6"""
    us = _system("PW", 20, 70, 9, 5)
    x, t0 = _data(48, 20, 70, seed=3)
    ref, _ = _oracle(us, x, t0)
    assert _err(torch.from_numpy(_flat(_run(us, x, t0), us)), ref, "PW V=70") <= TOL
    refk, _ = _oracle(us, x, t0, keep_tx=True)
    assert _err(torch.from_numpy(_flat(_run(us, x, t0, keep_tx=True), us)), refk, "PW V=70 keep_tx") <= TOL


def test_frequency_chunks_inside_a_workgroup(monkeypatch):
    """The summed kernel as a large image runs it.  I = 128 x 128 is 128 pixel tiles, so the 50 bins are cut into 512 / 128 = 4 chunks of 13, 13, 13
    and 11: a workgroup adds several frequencies in registers, the last chunk is ragged, the partial images are reduced in order.  Then with the fill
    target at 1: one chunk of all 50 bins per workgroup and `b` written directly, without the reduction; and at 2^20: one bin per workgroup."""
    us = _system("PW", 20, 7, 128, 128)
    x, t0 = _data(100, 20, 7, seed=10)
    ref, bins = _oracle(us, x, t0, fmod=2.5e6)
    assert len(bins) == 50 and int(np.prod(us.scan.size)) == 16384
    assert _err(torch.from_numpy(_flat(_run(us, x, t0, fmod=2.5e6), us)), ref, "I=128x128, 4 chunks of 13/13/13/11 bins") <= TOL
    refk, _ = _oracle(us, x, t0, fmod=2.5e6, keep_tx=True)
    assert _err(torch.from_numpy(_flat(_run(us, x, t0, fmod=2.5e6, keep_tx=True), us)), refk, "  keep_tx (norm pass in 4 chunks)") <= TOL
    monkeypatch.setenv("QDAS_ADJOINT_FILL", "1")
    assert _err(torch.from_numpy(_flat(_run(us, x, t0, fmod=2.5e6), us)), ref, "  one chunk of 50 bins, b written directly") <= TOL
    monkeypatch.setenv("QDAS_ADJOINT_FILL", str(1 << 20))
    assert _err(torch.from_numpy(_flat(_run(us, x, t0, fmod=2.5e6), us)), ref, "  one bin per workgroup") <= TOL


def test_unsplit_frequencies_at_a_small_image(core, monkeypatch):
    """the core shape (2 pixel tiles, the second partial) with every bin in one workgroup"""
    us, x, t0, ref, _ = core
    monkeypatch.setenv("QDAS_ADJOINT_FILL", "1")
    assert _err(torch.from_numpy(_flat(_run(us, x, t0, fmod=2.5e6), us)), ref, "core, one chunk of 48 bins") <= TOL
    monkeypatch.setenv("QDAS_ADJOINT_FILL", "10")                       # 10 / 2 = 5 chunks: ceil(48 / 5) = 10 bins each, the last 8
    assert _err(torch.from_numpy(_flat(_run(us, x, t0, fmod=2.5e6), us)), ref, "core, chunks of 10 and 8 bins") <= TOL


def test_a_zeroed_trace_does_not_change_the_bin_list():
    """a_mn is applied after the selection: a trace it zeroes still votes for its bins (reference :3935-3938 select on the un-apodized spectrum)"""
    us = _system("PW", 20, 7, 9, 5)
    x, t0 = _pulse_data(96, 20, 7)
    t = np.arange(96)[:, None] / FS
    x[:, 0, :] = (np.exp(-0.5 * ((t - 2e-6) / 0.15e-6) ** 2) * np.exp(2j * np.pi * 1.5e6 * (t - 2e-6))).astype(np.complex64)   # receiver 0 alone sits at 1.5 MHz ...
    amn = np.ones((1, 1, 1, 20, 7))
    amn[..., 0, :] = 0                                    # ... and a_mn removes it
    ref, bins = _oracle(us, x, t0, fthresh=-20.0, a_mn=amn[0, 0, 0])
    without = R.select_bins(R.spectrum(x[:, 1:], t0, FS), FS, -20.0)
    assert len(without) < len(bins)                       # receiver 0 is the only vote for some bins
    b, used = us.bfAdjoint(ChannelData(torch.from_numpy(x).cuda(), t0, FS), amn, fthresh=-20.0, return_bins=True)
    assert np.array_equal(used, bins)
    assert _err(torch.from_numpy(_flat(b, us)), ref, "a_mn zeroes the strongest receiver") <= TOL


@pytest.mark.parametrize("nz", [1, 33])
def test_single_element_single_transmit(nz):
    us = _system("PW", 1, 1, nz, 1)
    x, t0 = _data(64, 1, 1, seed=4)
    ref, _ = _oracle(us, x, t0)
    assert _err(torch.from_numpy(_flat(_run(us, x, t0), us)), ref, f"I={nz}, N=1, V=1") <= TOL


def test_fthresh_gives_a_ragged_frequency_list():
    us = _system("PW", 20, 7, 37, 5)
    x, t0 = _pulse_data(96, 20, 7)
    ref, bins = _oracle(us, x, t0, fthresh=-20.0)
    assert 1 < len(bins) < 96 // 2
    b, used = _run(us, x, t0, fthresh=-20.0, return_bins=True)
    assert np.array_equal(used, bins)
    assert _err(torch.from_numpy(_flat(b, us)), ref, f"fthresh -20: Ksel={len(bins)}") <= TOL


def test_nfft_longer_than_the_record():
    us = _system("PW", 20, 7, 37, 5)
    x, t0 = _data(80, 20, 7, seed=5)
    ref, bins = _oracle(us, x, t0, Nfft=128, fmod=1e6)
    assert len(bins) == 64
    assert _err(torch.from_numpy(_flat(_run(us, x, t0, Nfft=128, fmod=1e6), us)), ref, "T=80, Nfft=128") <= TOL


def test_sound_speed_scalar_and_map(core):
    us, x, t0, _, _ = core
    ref, _ = _oracle(us, x, t0, c0=1480.0)
    assert _err(torch.from_numpy(_flat(_run(us, x, t0, c0=1480.0), us)), ref, "c0 scalar") <= TOL
    cmap = 1500.0 + 80.0 * np.random.default_rng(6).uniform(size=us.scan.size)
    ref, _ = _oracle(us, x, t0, c0=cmap)
    assert _err(torch.from_numpy(_flat(_run(us, x, t0, c0=cmap), us)), ref, "c0 map") <= TOL


@pytest.mark.parametrize("which", ["a_n", "a_m", "a_mn", "a_n*a_m", "a_mn*a_n"])
def test_apodization_classes(core, which):
    us, x, t0, _, _ = core
    rng = np.random.default_rng(7)
    arr = {"a_n": rng.uniform(0.2, 1, (37, 5, 1, 20)), "a_m": rng.uniform(0.2, 1, (37, 1, 1, 1, 7)), "a_mn": rng.uniform(0.2, 1, (1, 1, 1, 20, 7))}
    use = which.split("*")
    kw = {}
    if "a_n" in use:
        kw["a_n"] = arr["a_n"]
    if "a_m" in use:
        kw["a_m"] = arr["a_m"][:, :, :, 0, :]
    if "a_mn" in use:
        kw["a_mn"] = arr["a_mn"][0, 0, 0]
    ref, _ = _oracle(us, x, t0, **kw)
    b = us.bfAdjoint(ChannelData(torch.from_numpy(x).cuda(), t0, FS), *[arr[k] for k in use])
    assert _err(torch.from_numpy(_flat(b, us)), ref, "apod " + which) <= TOL


def test_focused_transmits():
    us = _system("FC", 20, 3, 37, 5)
    x, t0 = _data(96, 20, 3, seed=8)
    assert np.all(us.seq.t0Offset() < 0) and np.asarray(us.seq.delays(us.tx)).min() > 0
    ref, _ = _oracle(us, x, t0, fmod=2.5e6)
    assert _err(torch.from_numpy(_flat(_run(us, x, t0, fmod=2.5e6), us)), ref, "FC, 3 foci") <= TOL


@pytest.mark.parametrize("keep_rx,keep_tx", [(False, True), (True, False), (True, True)])
def test_output_modes(core, keep_rx, keep_tx, monkeypatch):
    us, x, t0, ref, _ = core
    refk, _ = _oracle(us, x, t0, fmod=2.5e6, keep_rx=keep_rx, keep_tx=keep_tx)
    b = _run(us, x, t0, fmod=2.5e6, keep_rx=keep_rx, keep_tx=keep_tx)
    assert tuple(b.shape) == (37, 5, 1, 20 if keep_rx else 1, 7 if keep_tx else 1)
    assert _err(torch.from_numpy(_flat(b, us)), refk, f"keep_rx={keep_rx} keep_tx={keep_tx}") <= TOL
    s = b.sum(dim=(3, 4))
    assert _err(torch.from_numpy(s.cpu().numpy().reshape(-1, order="F")), ref, "  summed over the kept dimensions") <= TOL
    monkeypatch.setenv("QDAS_ADJOINT_BLOCK_BYTES", "20000")          # several pixel blocks, the last one partial
    b2 = _run(us, x, t0, fmod=2.5e6, keep_rx=keep_rx, keep_tx=keep_tx)
    assert _err(torch.from_numpy(_flat(b2, us)), refk, "  in pixel blocks") <= TOL


def test_frames_equal_single_frame_calls_bit_for_bit():
    us = _system("PW", 20, 7, 37, 5)
    x, t0 = _data(96, 20, 7, F=(3,), seed=9)
    b = _run(us, x, t0, fmod=2.5e6)
    assert tuple(b.shape) == (37, 5, 1, 3, 1, 1)
    for f in range(3):
        bf = _run(us, np.ascontiguousarray(x[..., f]), t0, fmod=2.5e6)
        assert torch.equal(b[:, :, :, f], bf)


def test_two_runs_are_bit_identical(core):
    us, x, t0, _, _ = core
    for kw in ({}, {"keep_tx": True}, {"keep_rx": True}):
        assert torch.equal(_run(us, x, t0, fmod=2.5e6, **kw), _run(us, x, t0, fmod=2.5e6, **kw))


def test_zero_sizes_launch_nothing():
    us = _system("PW", 20, 7, 37, 5)
    us.scan = Scan(np.zeros((3, 0, 1, 1)))
    x, t0 = _data(96, 20, 7)
    b = _run(us, x, t0)
    assert tuple(b.shape) == (0, 1, 1, 1, 1) and b.numel() == 0
    us2 = _system("PW", 20, 7, 5, 3)
    X = torch.zeros((0, 7, 20), dtype=torch.complex64, device="cuda")     # no frequency: an empty sum
    Pi = np.asarray(us2.scan.positions()).reshape(3, -1, order="F")
    b = A.adjoint(X, [], Pi, us2.rx.positions(), us2.tx.positions(), [1 / C0], us2.seq.delays(us2.tx), us2.seq.apodization(us2.tx))
    assert tuple(b.shape) == (15,) and not b.abs().any()


def test_return_delays(core):
    us, x, t0, _, _ = core
    b, tau_rx, tau_tx, tau_foc = _run(us, x, t0, return_delays=True)
    Pi = np.asarray(us.scan.positions(), float)
    for tau, P, shape in ((tau_rx, us.rx.positions(), (37, 5, 1, 20)), (tau_tx, us.tx.positions(), (37, 5, 1, 1, 20))):
        ref = np.linalg.norm(Pi[..., None] - np.asarray(P, float)[:, None, None, None, :], axis=0) / C0
        assert tuple(tau.shape) == shape
        assert np.abs(tau.cpu().numpy().reshape(ref.shape) - ref).max() <= 2.0 ** -23 * np.abs(ref).max()
    assert np.array_equal(tau_foc, np.asarray(us.seq.delays(us.tx)) + us.seq.t0Offset().reshape(1, -1))


def test_non_complex64_data_is_refused_by_the_library():
    from qups_amd import _lib
    X = torch.zeros((2, 3, 4), dtype=torch.complex128, device="cuda")
    with pytest.raises(DasError, match="complex128"):
        A.adjoint(X, [1.0, 2.0], np.zeros((3, 5)), np.zeros((3, 4)), np.zeros((3, 4)), [1.0], np.zeros((4, 3)), np.ones((4, 3)))
    assert _lib.lib() is not None
