"""Host side of refocus (no device): the float64 restatement (tests/refocus_ref.py) pinned by facts that follow from the formulas, the product's
``qups_amd.refocus.decoder`` against it, and the C ABI's symbols, descriptor and validation.

Bounds.  The Hadamard identity: 1e-12, about 1e3 eps T.  The decoders: a fixture asserts in float64 that every system solved has a condition of at most
1e4 and, for the random apodization, that every singular value lies at least 3 decades from the pinv cutoff; the bound is then 1e-9 (1e4 eps with two
decades of slack), on ``max|Hi - ref| / max|ref|``."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from qups_amd import DasError, _lib
from qups_amd import refocus as RF
from tests import refocus_ref as R
from tests.test_streams_host import stream_entries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 20e6


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


# ---------------------------------------------------------------------------------------------------------------- the restatement
def _hadamard_case(T=32, N=3, M=8, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, N, M)) + 1j * rng.standard_normal((T, N, M))
    a = R.hadamard(M)
    d = rng.integers(0, T // 2, M)
    tau = np.broadcast_to(d[None, :] / FS, (M, M))
    return x, a, d, tau


@pytest.mark.parametrize("method,gamma", [("adjoint", None), ("tikhonov", 0.0)])
def test_hadamard_identity(method, gamma):
    """a real Hadamard code with a common integer delay per pulse: refocus returns the FSA data.  The restatement, and the product's decoder applied by it."""
    x, a, d, tau = _hadamard_case()
    xe = R.hadamard_encode(x, a, d)
    y, t0, Hi = R.refocus(xe, 1.3e-6, FS, tau, a, method, gamma)
    assert y.shape == x.shape and t0 == 1.3e-6
    assert np.abs(y - x).max() <= 1e-12
    y2, _ = R.apply(xe, 1.3e-6, FS, RF.decoder(tau, a, 32, FS, method, gamma, 3))
    assert np.abs(y2 - x).max() <= 1e-12
    wrong = R.hadamard_encode(x, a, -d)                                  # the opposite shift direction is an O(1) error
    assert np.abs(R.apply(wrong, 0.0, FS, Hi)[0] - x).max() > 0.1


def test_pinv_does_not_satisfy_the_identity_and_matches_the_restatement_only():
    x, a, d, tau = _hadamard_case()
    xe = R.hadamard_encode(x, a, d)
    y, _, Hi = R.refocus(xe, 0.0, FS, tau, a, "pinv")
    assert np.abs(y - x).max() > 0.1                                     # H is the conjugate of the physical encoding (the reference: "not recommended")
    assert _rel(RF.decoder(tau, a, 32, FS, "pinv"), Hi) <= 1e-12


def test_the_frequency_axis_is_not_wrapped():
    """M = V = 1, a non-integer delay, adjoint: y = IDFT diag(exp(-2 pi i (k fs / T) tau)) DFT x with k = 0 .. T-1, evaluated with the T x T DFT matrix"""
    T, tau = 24, np.array([[3.37 / FS]])
    rng = np.random.default_rng(1)
    x = rng.standard_normal((T, 2, 1)) + 1j * rng.standard_normal((T, 2, 1))
    k = np.arange(T)
    F = np.exp(-2j * np.pi * np.outer(k, k) / T)
    direct = (np.conj(F) / T) @ (np.exp(-2j * np.pi * (k * FS / T) * tau[0, 0])[:, None] * (F @ x[:, :, 0]))
    y, _, Hi = R.refocus(x, 0.0, FS, tau, 1.0, "adjoint")
    assert _rel(y[:, :, 0], direct) <= 1e-12
    assert _rel(RF.decoder(tau, 1.0, T, FS, "adjoint")[0, 0], np.exp(-2j * np.pi * (k * FS / T) * tau[0, 0])) <= 1e-13
    kw = np.where(k < T / 2, k, k - T)                                   # the wrapped axis is a different operator
    wrapped = (np.conj(F) / T) @ (np.exp(-2j * np.pi * (kw * FS / T) * tau[0, 0])[:, None] * (F @ x[:, :, 0]))
    assert _rel(wrapped, direct) > 0.1
    # ... and a non-integer t0 fs per pulse (two pulses, one element, unit decoder rows): the same axis in step 5 and step 7
    t0 = np.array([2.0e-6, 2.0e-6 + 1.6 / FS])
    x2 = rng.standard_normal((T, 1, 2)) + 1j * rng.standard_normal((T, 1, 2))
    Hi2 = np.ones((1, 2, T), complex)
    y2, t0o = R.apply(x2, t0, FS, Hi2)
    ph = lambda t: np.exp(-2j * np.pi * (k * FS / T) * t)[:, None]
    direct2 = (np.conj(F) / T) @ ((ph(t0[0]) * (F @ x2[:, :, 0]) + ph(t0[1]) * (F @ x2[:, :, 1])) / ph(t0.min()))
    assert t0o == t0.min() and _rel(y2[:, :, 0], direct2) <= 1e-12


def test_pinv_of_the_all_ones_page():
    """tau = 0, unit apodization: every page is ones(V, M); pinv(ones) = ones / (V M), and with w = sigma_max^-2 = 1 / (V M) the decoder page is w times that"""
    M, V, T = 5, 3, 6
    for dec in (R.decoder, RF.decoder):
        Hi = dec(np.zeros((M, V)), np.ones((M, V)), T, FS, "pinv")
        assert np.allclose(Hi * (V * M), np.ones((M, V, T)) / (V * M), rtol=1e-12, atol=0)


@pytest.mark.parametrize("method", RF.METHODS)
def test_a_zero_page_gives_exactly_zero(method):
    tau = R.fc_sequence(4, 3)[0]
    for dec in (R.decoder, RF.decoder):
        Hi = dec(tau, np.zeros((4, 3)), 8, FS, method)
        assert Hi.shape == (4, 3, 8) and np.all(Hi == 0) and not np.isnan(Hi).any()


def test_default_gamma_and_shape():
    tau = R.fc_sequence(8, 6)[0]
    assert RF.default_gamma(64) == 10 * 6.4 ** 2 and R.default_gamma(64) == RF.default_gamma(64)
    Hi = RF.decoder(tau, 1.0, 48, FS, N=16)
    assert Hi.shape == (8, 6, 48) and Hi.dtype == np.complex128
    assert np.array_equal(Hi, RF.decoder(tau, 1.0, 48, FS, "tikhonov", 10 * 1.6 ** 2))
    assert np.array_equal(RF.decoder(tau, 1.0, 48, FS), RF.decoder(tau, 1.0, 48, FS, N=8))          # N defaults to M
    assert not np.array_equal(Hi, RF.decoder(tau, 1.0, 48, FS, N=32))
    with pytest.raises(DasError, match="method"):
        RF.decoder(tau, 1.0, 48, FS, "ridge")
    with pytest.raises(DasError, match="gamma"):
        RF.decoder(tau, 1.0, 48, FS, gamma=-1.0)
    with pytest.raises(DasError, match="broadcast"):
        RF.decoder(tau, np.ones((3, 3)), 48, FS)


def test_per_pulse_t0_with_integer_offsets_is_a_circular_shift():
    """pulse v recorded from t0 + j_v / fs is pulse v recorded from t0 and delayed by j_v samples (circularly: the method is periodic)"""
    T, N, M, V = 40, 2, 4, 3
    rng = np.random.default_rng(2)
    x = rng.standard_normal((T, N, V)) + 1j * rng.standard_normal((T, N, V))
    tau = R.fc_sequence(M, V)[0]
    j = np.array([0, 5, 2])
    Hi = R.decoder(tau, 1.0, T, FS, "tikhonov", None, N)
    ya, ta = R.apply(x, 1e-6 + j / FS, FS, Hi)
    xs = np.stack([np.roll(x[:, :, v], j[v], axis=0) for v in range(V)], axis=2)
    yb, tb = R.apply(xs, 1e-6, FS, Hi)
    assert ta == tb == 1e-6 and _rel(ya, yb) <= 1e-12


def test_end_to_end_the_restatement_meets_the_reference_criterion():
    """reference test/BFTest.m:309-316 on the geometry tests/test_gpu_refocus.py runs on the device: FSA data (tests/golden F2) -> focusTx to 17 plane waves ->
    zero-pad -> refocus (the restatement) -> FSA DAS (the oracle): the image peaks within 1.1 mm of the scatterer in x and in z"""
    from oracle import das_oracle as O
    from qups_amd import geometry as G
    g = np.load(os.path.join(ROOT, "tests", "golden", "f2_psf.npz"))
    x, t0, fs, Pr, c0, scat = g["FSA_x"].astype(complex), float(g["FSA_t0"]), float(g["FSA_fs"]), g["FSA_Pr"], float(g["FSA_c"]), g["FSA_scat"]
    tau = O.sequence_delays("PW", Pr, R.pw_normals(R.E2E_ANGLES), c0)
    z, t0z = O.focus_tx(x, t0, fs, tau, 1.0, "cubic")
    zp, t0p = O.zeropad(z, t0z, fs, R.E2E_PAD, R.pad_behind(z.shape[0], RF.takes))
    assert RF.takes(zp.shape[0])
    Pv, Nv, _ = G.sequence_args("FSA", tx_pos=Pr, tx_normals=np.tile(np.array([[0.0], [0.0], [1.0]]), (1, Pr.shape[1])))
    for method in ("adjoint", "tikhonov"):
        y, t0y, _ = R.refocus(zp, float(t0p), fs, tau, 1.0, method)
        b = np.abs(O.das_spec("DAS", G.scan_cartesian(R.E2E_X, R.E2E_Z), Pr, Pv, Nv, y, t0y, fs, c0, VS=True, DV=True, interp="cubic"))[:, :, 0, 0, 0]
        iz, ix = np.unravel_index(np.argmax(b), b.shape)
        assert b.max() > 0 and abs(R.E2E_X[ix] - scat[0]) <= 1.1e-3 and abs(R.E2E_Z[iz] - scat[2]) <= 1.1e-3, (method, R.E2E_X[ix], R.E2E_Z[iz])


# ---------------------------------------------------------------------------------------------------------------- the product's decoder
M_FC, T_FC = 8, 48


def _apd(kind, V):
    return np.ones((M_FC, V)) if kind == "unit" else np.random.default_rng(7).uniform(0.5, 1.5, (M_FC, V))


@pytest.fixture(scope="module")
def conditioning():
    """float64, CPU: every tikhonov system of the cases below has a condition of at most 1e4; with the random apodization every singular value of every
    page lies at least 3 decades above the pinv cutoff max(V, M) eps(sigma_max)"""
    out = {}
    for V in (6, 10):
        tau = R.fc_sequence(M_FC, V)[0]
        for kind in ("unit", "random"):
            info = {}
            R.decoder(tau, _apd(kind, V), T_FC, FS, "tikhonov", None, None, info)
            assert info["cond"].max() <= 1e4, (V, kind, info["cond"].max())
            if kind == "random":
                decades = min(np.log10(s.min() / (max(V, M_FC) * np.spacing(s[0]))) for s in info["svals"])
                assert decades >= 3, (V, decades)
                out[V] = decades
    return out


@pytest.mark.parametrize("V", [6, 10])
@pytest.mark.parametrize("kind,method", [("unit", "adjoint"), ("unit", "tikhonov"), ("random", "adjoint"), ("random", "tikhonov"), ("random", "pinv")])
def test_decoder_matches_the_restatement(conditioning, V, kind, method):
    tau, apd = R.fc_sequence(M_FC, V)[0], _apd(kind, V)
    got, ref = RF.decoder(tau, apd, T_FC, FS, method), R.decoder(tau, apd, T_FC, FS, method)
    assert got.shape == ref.shape == (M_FC, V, T_FC)
    e = _rel(got, ref)
    print(f"decoder M={M_FC} V={V} {kind} {method}: rel_err={e:.3e} (pinv margin {conditioning[V]:.1f} decades)")
    assert e <= 1e-9


def test_decoder_object_checks_its_shape():
    with pytest.raises(DasError, match="M x V x T"):
        RF.Decoder(np.zeros((3, 4)))
    d = RF.Decoder(np.zeros((3, 4, 5), np.complex64))
    assert (d.M, d.V, d.T) == (3, 4, 5) and d.Hi.dtype == np.complex128


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_abi_symbols_and_descriptor():
    L = _lib.lib()
    for s in ("qdas_refocus", "qdas_refocus_work_bytes"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
    D = _lib.RefocusDesc
    assert C.sizeof(D) == 80                                            # 5 extents, 2 doubles, 2 ints, 2 pointers
    assert (D.frames.offset, D.fs.offset, D.t0_out.offset, D.device.offset, D.one_t0.offset, D.t0.offset, D.queue.offset) == (32, 40, 48, 56, 60, 64, 72)
    assert L.qdas_version() == 103
    assert "refocus" in __import__("qups_amd").__all__ and callable(RF.refocus) and callable(RF.compose)


def _desc(**kw):
    d = _lib.RefocusDesc()
    d.T, d.N, d.V, d.M, d.frames = 64, 5, 6, 8, 1
    d.fs, d.t0_out, d.device, d.one_t0 = FS, 0.0, -1, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


BUF = (C.c_double * 8)()
P = C.cast(BUF, C.c_void_p)


def _need(d):
    n = C.c_uint64()
    assert _lib.lib().qdas_refocus_work_bytes(C.byref(d), C.byref(n)) == 0
    return n.value


def test_work_bytes():
    d = _desc()
    tw = (64 * 8 + 255) // 256 * 256
    assert _need(d) == tw + 8 * 64 * 5 * (6 + 8)
    assert _need(_desc(frames=3)) == tw + 8 * 64 * 15 * (6 + 8)
    assert _need(_desc(T=0)) == 0
    L = _lib.lib()
    n = C.c_uint64()
    assert L.qdas_refocus_work_bytes(None, C.byref(n)) == 1 and L.qdas_refocus_work_bytes(C.byref(d), None) == 1
    assert L.qdas_refocus_work_bytes(C.byref(_desc(T=34)), C.byref(n)) == _lib.QDAS_ENOTLDS and n.value == 0


@pytest.mark.parametrize("args,kw,code,text", [
    ((None, P, P, P), {}, 1, "null data pointer"), ((P, None, P, P), {}, 1, "null data pointer"), ((P, P, None, P), {}, 1, "null data pointer"),
    ((P, P, P, None), {}, 1, "null data pointer"), ((P, P, P, P), dict(one_t0=0), 1, "null data pointer"),
    ((P, P, P, P), dict(work=-1), 1, "work space holds"), ((P, P, P, P), dict(work=0), 1, "work space holds"),
    ((P, P, P, P), dict(T=34), 6, "in-LDS"), ((P, P, P, P), dict(T=8193), 6, "in-LDS"), ((None, None, None, None), dict(T=1), 6, "in-LDS"),
    ((P, P, P, P), dict(T=8192 * 3), 6, "in-LDS"),
    ((P, P, P, P), dict(V=65536), 2, "65535"), ((P, P, P, P), dict(N=1 << 31), 2, "extent"), ((P, P, P, P), dict(N=1 << 20, frames=1 << 12), 2, "N \\* frames"),
    ((P, P, P, P), dict(fs=0.0), 1, "fs"), ((P, P, P, P), dict(t0_out=float("nan")), 1, "t0_out"), ((P, P, P, P), dict(one_t0=2), 1, "one_t0"),
])
def test_c_abi_rejects_bad_calls_before_any_launch(args, kw, code, text):
    """device = -1 and pointers to host memory: nothing here may reach a HIP call"""
    L = _lib.lib()
    kw = dict(kw)
    work = kw.pop("work", None)
    d = _desc(**kw)
    nbytes = 1 << 40
    if work is not None:
        nbytes = _need(d) + work if work < 0 else work
    assert L.qdas_refocus(C.byref(d), *args, nbytes) == code
    assert re.search(text, L.qdas_last_error().decode())


def test_c_abi_null_descriptor_empty_problem_and_routing_code():
    L = _lib.lib()
    assert L.qdas_refocus(None, P, P, P, P, 0) == 1
    for kw in (dict(T=0), dict(N=0), dict(V=0), dict(M=0), dict(frames=0)):
        assert L.qdas_refocus(C.byref(_desc(**kw)), None, None, None, None, 0) == 0          # nothing to do, no device needed
    assert _lib.QDAS_ENOTLDS == 6
    assert RF.takes(64) and RF.takes(8192) and RF.takes(77) and RF.takes(48) and not RF.takes(34) and not RF.takes(1) and not RF.takes(8193)


def test_the_stream_travels_in_the_descriptor_and_has_its_case_in_the_gpu_file():
    """the census of ``void *stream`` parameters (tests/test_streams_host.py) is a pinned list: qdas_refocus takes its stream in ``queue`` and its stream
    cases live in tests/test_gpu_refocus.py"""
    with open(os.path.join(ROOT, "include", "qdas.h")) as f:
        header = f.read()
    assert "qdas_refocus" not in stream_entries(header) and "qdas_refocus_work_bytes" not in stream_entries(header)
    assert re.search(r"void\s*\*\s*queue\s*;", header)
    from tests import test_gpu_refocus as G
    for name in G.STREAM_CASES:
        assert name.startswith("test_") and callable(getattr(G, name))
    assert len(G.STREAM_CASES) >= 2
    with open(os.path.join(ROOT, "qups_amd", "csrc", "refocus.hip")) as f:
        src = f.read()
    from tests.test_scratch_host import scratch_users
    assert not scratch_users(src)                                        # the work space is the caller's: no arena of the library
