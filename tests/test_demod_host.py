"""qdas_demod without a GPU: the restatement tests/demod_ref.py against a direct triple loop and the formulas of the three ChannelData methods it fuses, the
time-axis rule, the C entry's validation (``device = -1``: nothing reaches a HIP call), the descriptor against the header, the two filter designers against
their closed form, and the kernel's index and phase arithmetic (``csrc/demod_core.h``) walked on the CPU by a stand-alone program under AddressSanitizer and
UBSan (tests/demod_core_host.cpp) against the restatement.

The program evaluates in the kernel's order and precision, so its error is the "emulation of the intended evaluation order".  In the units of the GPU test's
bound, ``err / (eps sum|b| max|x|)`` against ``K + 8``: the first six rows of ``CORE_CASES`` are float32 shapes up to K = 129, five with real input and one
with complex input.  The five real ones give 0.3 - 0.8; the complex one (K = 2, whose phase roundings weigh more beside two taps) gives 1.4.
THIS DIFFERS FROM THE ISSUE, which states that such an emulation stays below 1.0 eps for six shapes: that holds for the real shapes only, not for complex
input with few taps.  The bound itself (K + 8 = 10 units there) is not touched by this.  What the test asserts is not the quoted figure either: every case
must stay below HALF the GPU test's bound, the other half being room for the device's math library."""
import ctypes as C
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

from qups_amd import _lib
from tests import demod_ref as R
from tests.test_streams_host import stream_entries

DM = importlib.import_module("qups_amd.demod")            # (the package exports the function under the module's name)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FC, FS = 5.1e6, 20e6


def _x(T, Cn, cplx=False, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, Cn))
    return x + 1j * rng.standard_normal((T, Cn)) if cplx else x


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("T,K,ratio,cplx", [(1, 1, 1, False), (7, 3, 2, False), (23, 5, 4, True), (9, 12, 3, False), (16, 4, 8, True), (5, 2, 7, False)])
def test_restatement_against_the_triple_loop(T, K, ratio, cplx):
    x, b = _x(T, 3, cplx), np.random.default_rng(K).standard_normal(K)
    t0 = np.array([1.1e-6, -0.4e-6, 0.0])
    got = R.demod(x, FC, FS, t0.reshape(1, 3), b, ratio)
    want = R.demod_loops(x, FC, FS, t0, b, ratio)
    assert got.shape == want.shape == (-(-T // ratio), 3)
    assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max())


def test_restatement_against_the_three_methods_formulas():
    """downmix: data .* exp(-2i pi fc time); filter: MATLAB's causal filter (scipy.signal.lfilter); downsample: 1:ratio:T"""
    from scipy.signal import lfilter
    T, K, ratio = 41, 6, 4
    x, b = _x(T, 2), np.random.default_rng(1).standard_normal(K)
    t0 = 2.3e-6
    time = t0 + np.arange(T)[:, None] / FS
    mixed = x * np.exp(-2j * np.pi * FC * time)
    want = lfilter(b, [1.0], mixed, axis=0)[::ratio]
    assert np.abs(R.demod(x, FC, FS, t0, b, ratio) - want).max() <= 1e-12
    assert np.abs(R.downmix(x, FC, FS, t0) - mixed).max() <= 1e-12
    assert np.array_equal(R.downsample(np.arange(10), 4), [0, 4, 8])


def test_time_axis_rule():
    t0, fs = R.time_axis(1e-6, 20e6, 25, 4)
    assert float(t0) == 1e-6 - 12 / 20e6 and fs == 5e6
    t0v = np.array([1e-6, 2e-6]).reshape(1, 1, 2)
    t0n, _ = R.time_axis(t0v, 20e6, 26, 2)
    assert t0n.shape == (1, 1, 2) and np.array_equal(t0n, t0v - 12.5 / 20e6)
    assert DM.demod_len(2816, 4) == 704 and DM.demod_len(5, 4) == 2 and DM.demod_len(4, 4) == 1 and DM.demod_len(0, 3) == 0


def test_start_groups():
    v, gdiv, G = DM.start_groups(0.5, (3, 2))
    assert (v.tolist(), gdiv, G) == ([0.5], 1, 1)
    v, gdiv, G = DM.start_groups(np.array([1.0, 2.0]).reshape(1, 2), (3, 2))
    assert (v.tolist(), gdiv, G) == ([1.0, 2.0], 1, 2)                       # row-major traces: c = n * 2 + m
    v, gdiv, G = DM.start_groups(np.array([1.0, 2.0]).reshape(1, 2, 1), (3, 2, 5))
    assert (v.tolist(), gdiv, G) == ([1.0, 2.0], 5, 2)
    v, gdiv, G = DM.start_groups(np.arange(6.0).reshape(3, 2), (3, 2))
    assert (gdiv, G) == (1, 6) and v.tolist() == list(range(6))
    with pytest.raises(DM.DasError):
        DM.start_groups(np.zeros(4), (3, 2))
    c = DM.start_cycles(5e6, [-1.1e-6, 0.3e-6])
    assert ((c >= 0) & (c < 1)).all() and abs(c[1] - 0.5) < 1e-12 and abs(c[0] - 0.5) < 1e-9


# ---------------------------------------------------------------------------------------------------------------- the filter designers
def _hamming(n):
    return 0.54 - 0.46 * np.cos(2 * np.pi * np.arange(n) / (n - 1))


@pytest.mark.parametrize("N,cutoff", [(25, 2e6), (24, 3.3e6), (128, 1e6)])
def test_lowpass_taps_are_the_windowed_sinc(N, cutoff):
    from qups_amd import ChannelData
    b = ChannelData(np.zeros((4, 1, 1)), 0.0, FS).getLowpassFilter(cutoff, N)
    n = np.arange(N + 1) - N / 2
    h = 2 * cutoff / FS * np.sinc(2 * cutoff / FS * n) * _hamming(N + 1)
    h /= h.sum()
    assert b.shape == (N + 1,) and np.abs(b - h).max() <= 1e-15
    assert abs(b.sum() - 1) <= 1e-14 and np.abs(b - b[::-1]).max() <= 1e-16


@pytest.mark.parametrize("N,band", [(25, (3e6, 7e6)), (64, (4e6, 6e6))])
def test_passband_taps_are_the_difference_of_two_windowed_sincs(N, band):
    from qups_amd import ChannelData
    b = ChannelData(np.zeros((4, 1, 1)), 0.0, FS).getPassbandFilter(band, N)
    n = np.arange(N + 1) - N / 2
    f1, f2 = (2 * f / FS for f in band)
    h = (f2 * np.sinc(f2 * n) - f1 * np.sinc(f1 * n)) * _hamming(N + 1)
    centre = (f1 + f2) / 2
    h /= np.sum(h * np.cos(np.pi * n * centre))
    assert b.shape == (N + 1,) and np.abs(b - h).max() <= 1e-14
    assert np.abs(b - b[::-1]).max() <= 1e-16
    assert abs(abs(np.sum(b * np.exp(-1j * np.pi * np.arange(N + 1) * centre))) - 1) <= 1e-13


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_abi_symbols_and_descriptor_layout():
    L = _lib.lib()
    for s in ("qdas_demod", "qdas_demod_len"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
    D = _lib.DemodDesc
    assert C.sizeof(D) == 6 * 8 + 4 * 4 + 2 * 8 + 8 + 2 * 8 + 8
    assert (D.x_ld.offset, D.in_type.offset, D.device.offset, D.fc_over_fs.offset, D.cyc0.offset, D.gdiv.offset, D.queue.offset) == (32, 48, 56, 64, 80, 88, 104)
    with open(os.path.join(ROOT, "include", "qdas.h")) as f:
        header = f.read()
    body = re.search(r"typedef struct qdas_demod_desc \{(.*?)\} qdas_demod_desc;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            rest = decl.split(None, 1 + decl.startswith("const"))[-1]
            names += [n.strip(" *") for n in rest.split(",")]
    assert names == [n for n, _ in D._fields_]
    codes = tuple(int(re.search(rf"#define QDAS_DEMOD_{n}\s+(\d+)", header).group(1)) for n in ("I16", "F32", "C64", "F64", "C128", "MAX_K", "MAX_R", "TILE"))
    assert codes == (_lib.DEMOD_I16, _lib.DEMOD_F32, _lib.DEMOD_C64, _lib.DEMOD_F64, _lib.DEMOD_C128, _lib.DEMOD_MAX_K, _lib.DEMOD_MAX_R, _lib.DEMOD_TILE)
    assert _lib.DEMOD_MAX_K >= 1024 and _lib.DEMOD_MAX_R >= 64
    import qups_amd
    assert "demod" in qups_amd.__all__ and callable(qups_amd.demod)


def test_demod_len():
    L = _lib.lib()
    for T, ratio, want in ((0, 1, 0), (1, 1, 1), (1, 4, 1), (4, 4, 1), (5, 4, 2), (2816, 4, 704), (3, 0, 0), ((1 << 40) + 1, 1 << 20, (1 << 20) + 1)):
        assert L.qdas_demod_len(T, ratio) == want, (T, ratio)


BUF = (C.c_double * 8)()
P = C.cast(BUF, C.c_void_p)


def _desc(**kw):
    d = _lib.DemodDesc()
    d.T, d.C, d.K, d.R, d.x_ld, d.out_ld = 100, 2, 5, 4, 100, 25
    d.in_type, d.out_half, d.device = _lib.DEMOD_F32, 0, -1
    d.fc_over_fs, d.step, d.gdiv, d.G, d.cyc0 = 0.25, 1.0, 1, 1, P
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("kw,code,text", [
    (dict(R=0), 1, "ratio R"), (dict(K=0), 1, "at least one tap"), (dict(x_ld=99), 1, "x_ld"), (dict(out_ld=24), 1, "out_ld"),
    (dict(in_type=5), 1, "in_type"), (dict(in_type=-1), 1, "in_type"), (dict(out_half=2), 1, "out_half"), (dict(out_half=-1), 1, "out_half"),
    (dict(in_type=_lib.DEMOD_F64, out_half=1), 1, "double data"), (dict(in_type=_lib.DEMOD_C128, out_half=1), 1, "double data"),
    (dict(G=0), 1, "G and gdiv"), (dict(gdiv=0), 1, "G and gdiv"),
    (dict(fc_over_fs=math.nan), 1, "finite"), (dict(fc_over_fs=math.inf), 1, "finite"), (dict(step=-math.inf), 1, "finite"), (dict(step=math.nan), 1, "finite"),
    (dict(cyc0=None), 1, r"null pointer \(cyc0\)"),
    (dict(K=_lib.DEMOD_MAX_K + 1), 2, "taps"), (dict(R=_lib.DEMOD_MAX_R + 1), 2, "ratio"),
    (dict(T=1 << 40, x_ld=1 << 40, out_ld=1 << 40), 2, "2\\^40"), (dict(C=1 << 31), 2, "workgroups"), (dict(T=1 << 39, x_ld=1 << 39, out_ld=1 << 39, C=2, R=1), 2, "workgroups"),
])
def test_c_abi_rejects_bad_calls_before_any_launch(kw, code, text):
    """device = -1 and pointers to host memory: nothing here may reach a HIP call"""
    L = _lib.lib()
    assert L.qdas_demod(C.byref(_desc(**kw)), P, P, P) == code
    assert re.search(text, L.qdas_last_error().decode()), L.qdas_last_error()


def test_c_abi_null_pointers_and_empty_problems():
    L = _lib.lib()
    assert L.qdas_demod(None, P, P, P) == 1 and "null descriptor" in L.qdas_last_error().decode()
    for args, what in (((None, P, P), "x"), ((P, None, P), "b"), ((P, P, None), "out")):
        assert L.qdas_demod(C.byref(_desc()), *args) == 1 and f"null pointer ({what})" in L.qdas_last_error().decode()
    for kw in (dict(T=0), dict(C=0), dict(T=0, C=0, x_ld=0, out_ld=0)):
        assert L.qdas_demod(C.byref(_desc(cyc0=None, **kw)), None, None, None) == 0            # nothing to do, no device needed
    assert L.qdas_demod(C.byref(_desc(T=0, R=0)), None, None, None) == 1, "an empty call is still validated"
    assert L.qdas_demod(C.byref(_desc(K=_lib.DEMOD_MAX_K, R=_lib.DEMOD_MAX_R)), None, P, P) == 1 and "null pointer" in L.qdas_last_error().decode()   # the limits themselves are taken


def test_the_stream_travels_in_the_descriptor_and_there_is_no_work_space():
    with open(os.path.join(ROOT, "include", "qdas.h")) as f:
        header = f.read()
    assert not [n for n in stream_entries(header) if "demod" in n]
    proto = re.search(r"\bint\s+qdas_demod\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1)
    assert "stream" not in proto and "qdas_demod_desc" in proto and proto.count(",") == 3
    from tests import test_gpu_demod as GDm
    assert callable(GDm.test_stream_delayed_producer_on_a_side_stream)
    from tests.test_scratch_host import scratch_users
    for fn in ("demod.hip", "demod_core.h"):
        with open(os.path.join(ROOT, "qups_amd", "csrc", fn)) as f:
            src = f.read()
        assert not scratch_users(src) and "hipMalloc" not in src and "Synchronize" not in src and "atomic" not in re.sub(r"//[^\n]*", "", src)
    with open(os.path.join(ROOT, "qups_amd", "csrc", "demod_core.h")) as f:
        assert "hip/" not in f.read(), "the core has no HIP dependency"
    with open(os.path.join(ROOT, "qups_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert " demod.hip" in mk and " demod_core.h" in mk


def test_python_argument_handling_without_a_device():
    import torch
    with pytest.raises(DM.DasError, match="device tensor"):
        DM.demod(torch.zeros(8, 2), FC, FS, 0.0, [1.0], 2)
    with pytest.raises(DM.DasError, match="device tensor"):
        DM.demod(np.zeros((8, 2)), FC, FS, 0.0, [1.0], 2)
    with pytest.raises(DM.DasError):
        DM.lowpass_taps(11e6, FS)
    with pytest.raises(DM.DasError):
        DM.passband_taps((7e6, 3e6), FS)


# ---------------------------------------------------------------------------------------------------------------- the device's core, on the host
@pytest.fixture(scope="module")
def core_exe(tmp_path_factory):
    """demod_core.h under AddressSanitizer and UBSan in a stand-alone program: taps, rows and records are heap blocks of exactly their size"""
    exe = str(tmp_path_factory.mktemp("dm") / "demod_core_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "qups_amd", "csrc"), os.path.join(ROOT, "tests", "demod_core_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _fmt(v):
    return " ".join(float(t).hex() for t in np.asarray(v, np.float64).reshape(-1))


def run_core(exe, tmp_path, x, b, ratio, cyc0, gdiv, bits):
    """``(out J x C, geometry line)``; x: T x C in the values the program is to see"""
    T, Cn = x.shape
    cplx = int(np.iscomplexobj(x))
    path = str(tmp_path / "case.txt")
    cyc0 = np.atleast_1d(cyc0)
    with open(path, "w") as f:
        f.write(f"{bits} {cplx} {T} {Cn} {len(b)} {ratio} {(FC / FS).hex()} {(FC / FS * ratio).hex()} {cyc0.size} {gdiv}\n")
        f.write(_fmt(cyc0) + "\n" + _fmt(b) + "\n")
        flat = np.asarray(x).T.reshape(-1)
        f.write(_fmt(np.stack([flat.real, flat.imag], 1) if cplx else flat) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    geom = dict(zip(("S", "NG", "QP", "EN", "PG", "lds", "loads_max"), (int(v) for v in lines[0].split())))
    val = np.array([complex(float.fromhex(a), float.fromhex(c)) for a, c in (ln.split() for ln in lines[1:])])
    return val.reshape(Cn, -(-T // ratio)).T, geom


CORE_CASES = [   # T, C, K, ratio, cplx, bits: six float32 shapes up to K = 129 (five real, the sixth complex), then the corners of the layout
    (700, 2, 25, 4, 0, 32), (1100, 1, 129, 4, 0, 32), (900, 1, 26, 3, 0, 32), (600, 1, 129, 1, 0, 32), (2100, 1, 33, 8, 0, 32), (530, 2, 2, 2, 1, 32),
    (1, 1, 1, 1, 0, 32), (5, 1, 9, 4, 0, 64), (300, 1, 300, 1, 0, 32), (2060, 1, 7, 8, 0, 32), (2400, 1, 40, 9, 1, 64), (4700, 1, 35, 16, 0, 32),
    (1300, 1, 1024, 1, 1, 64), (3 * 4096 + 5, 1, 33, 4096, 0, 32), (64 * 3 + 1, 1, 1024, 64, 0, 32), (257 * 3, 1, 5, 3, 0, 64),
]


@pytest.mark.parametrize("T,Cn,K,ratio,cplx,bits", CORE_CASES)
def test_the_core_on_the_host_matches_the_restatement(core_exe, tmp_path, T, Cn, K, ratio, cplx, bits):
    rt = np.float32 if bits == 32 else np.float64
    x = _x(T, Cn, bool(cplx), seed=T + K)
    x = (x.real.astype(rt) + 1j * x.imag.astype(rt)) if cplx else x.astype(rt).astype(np.float64)
    b = (np.random.default_rng(K).standard_normal(K) / np.sqrt(K)).astype(rt).astype(np.float64)
    t0 = np.array([3.3e-6, -1.7e-6])[:Cn]
    got, geom = run_core(core_exe, tmp_path, x, b, ratio, DM.start_cycles(FC, t0), 1, bits)
    want = R.demod(x, FC, FS, t0.reshape(1, -1), b, ratio)
    assert geom["S"] == min(ratio, K) and 1 <= geom["PG"] <= 8 and geom["lds"] <= 65536 and geom["QP"] >= geom["NG"] + 64
    assert geom["loads_max"] <= (4 * geom["NG"] + 255) // 256 + 1, "a sample is staged once per tile whose rows hold it"
    eps = 2.0 ** -24 if bits == 32 else 2.0 ** -53
    err = np.abs(got - want).max()
    units = err / (np.abs(b).sum() * np.abs(x).max()) / eps
    bd = R.bound(K, b, np.abs(x).max(), FC * (np.abs(t0).max() + T / FS), double=bits == 64)
    print(f"demod core {T} x {Cn}, K = {K}, R = {ratio}, {bits} bit: {units:.3f} eps of sum|b| max|x| (K + 8 = {K + 8}), {err / bd:.3f} of the bound")
    assert err <= 0.5 * bd, "half the GPU test's bound: the other half is room for the device's math library"


def test_the_core_reads_no_sample_without_a_tap(core_exe, tmp_path):
    """R = 8, K = 3: indices = 1 .. 5 (mod 8) are NaN and the result is finite -- they are neither loaded into a row that is read nor multiplied by zero;
    one NaN elsewhere reaches exactly the outputs of the contract"""
    T, K, ratio = 2100, 3, 8
    x = _x(T, 1, seed=8).astype(np.float32).astype(np.float64)
    b = np.array([0.5, -0.25, 0.125])
    clean, _ = run_core(core_exe, tmp_path, x, b, ratio, 0.3, 1, 32)
    idx = np.arange(T)
    y = x.copy()
    y[(idx % 8 >= 1) & (idx % 8 <= 5)] = np.nan
    got, _ = run_core(core_exe, tmp_path, y, b, ratio, 0.3, 1, 32)
    assert np.isfinite(got).all() and np.array_equal(got, clean)
    y = x.copy()
    y[1031] = np.nan                                                   # 1031 = 8 * 129 - 1: read by output 129 alone
    got, _ = run_core(core_exe, tmp_path, y, b, ratio, 0.3, 1, 32)
    hit = np.zeros(got.shape[0], bool)
    hit[R.nan_reach(1031, K, ratio, got.shape[0])] = True
    assert hit.sum() == 1 and hit[129] and np.isnan(got[hit]).all() and np.array_equal(got[~hit], clean[~hit])


def core_map(exe, K, ratio, eb, cb):
    """``(NG, QP, EN, pg, words[pg][EN], first store word of every lane)`` as demod_core.h computes them (the program's ``map`` mode)"""
    r = subprocess.run([exe, "map", str(K), str(ratio), str(eb), str(cb)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    head, words, first = r.stdout.strip().split("\n")
    NG, QP, EN, pg = (int(v) for v in head.split())
    return NG, QP, EN, pg, np.array(words.split(), np.int64).reshape(pg, EN), np.array(first.split(), np.int64)


@pytest.mark.parametrize("K,ratio,eb,cb", [(25, 4, 4, 8), (129, 4, 4, 8), (1024, 1, 16, 16), (33, 8, 8, 8), (33, 8, 8, 16), (1024, 64, 4, 8), (5, 3, 4, 8)])
def test_the_lds_map_is_one_to_one_and_spreads_the_stores(core_exe, K, ratio, eb, cb):
    """the header's own ``lds_word`` / ``plane_len`` / ``geometry``, printed by the stand-alone program: every (phase, element) of a staging group has its own
    word inside the rows, a plane holds the quads the window reads, and for 4-byte samples and R = 4 the 32 lanes of a store group hit 32 different banks"""
    NG, QP, EN, pg, words, first = core_map(core_exe, K, ratio, eb, cb)
    assert NG == (K - 1) // ratio // 4 + 1 and EN == 4 * (NG + 64) and pg == min(ratio, K, 8)
    assert QP >= NG + 64 and QP % (32 if eb == 4 else 16) == (2 if eb == 4 else 1) and QP - (NG + 64) < (32 if eb == 4 else 16)
    assert len(np.unique(words)) == words.size and words.min() >= 0 and words.max() < pg * 4 * QP
    assert np.array_equal(first, [words[t % pg, t // pg] for t in range(64)])
    if (ratio, eb) == (4, 4):
        for lanes in (first[:32], first[32:]):
            assert len(set(lanes % 32)) == 32


def test_gateway_compiles_and_links():
    """mex/qdas_mex.c with the 'demod' command against the fake MEX API of tests/fake_mex (the run itself needs a GPU: tests/test_mex_demod.py)"""
    from tests import test_mex_demod as M
    exe = M.build_gateway()
    assert os.path.exists(exe)
