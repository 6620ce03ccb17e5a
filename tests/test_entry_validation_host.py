"""The one-shot entries of the C ABI without a device: what each of them rejects before its first HIP call (return code and the text of
qdas_last_error()), qdas_convd_len, and the library's symbol table against include/qdas.h.  Every descriptor says device = -1, so no entry
switches devices on the way to the rejection."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from qups_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
BUF = C.c_void_p(1)          # a non-null pointer no entry may touch


def _rejects(rc, text):
    assert rc == EINVAL, (rc, _lib.lib().qdas_last_error())
    assert _lib.lib().qdas_last_error() == text


def test_das_lut_rejects_unknown_precision_and_interpolator():
    L = _lib.lib()
    d = _lib.LutDesc()
    d.T, d.N, d.M, d.I, d.flag, d.dtype = 16, 2, 2, 8, 1, 3
    _rejects(L.qdas_das_lut(C.byref(d), BUF, BUF, None), b"Unrecognized input precision 3")
    d.dtype = -1
    _rejects(L.qdas_das_lut(C.byref(d), BUF, BUF, None), b"Unrecognized input precision -1")
    d.dtype, d.flag = _lib.QDAS_F32, 6 | _lib.FLAG_KEEP_RX
    _rejects(L.qdas_das_lut(C.byref(d), BUF, BUF, None), b"Interp option not recognized: 6")


def test_wsinterpd_rejects_no_dimensions_and_a_strided_sampling_dimension():
    L = _lib.lib()
    d = _lib.WsDesc()
    d.T, d.ndim, d.flag, d.dtype = 16, 0, 1, _lib.QDAS_F32
    _rejects(L.qdas_wsinterpd(C.byref(d), BUF, None), b"wsinterpd: 1..8 dimensions")
    d.ndim = 2
    d.size[0], d.size[1], d.tstride[0], d.tstride[1], d.xstride[0], d.xstride[1] = 4, 3, 1, 4, 1, 16
    _rejects(L.qdas_wsinterpd(C.byref(d), BUF, None), b"wsinterpd: xstride[0] must be 0 (dimension 0 is the sampling dimension)")


def test_greens_rejects_zero_element_subdivisions():
    L = _lib.lib()
    d = _lib.GreensDesc()
    d.S, d.T, d.N, d.M, d.I = 8, 16, 2, 2, 3
    d.En, d.Em, d.interp, d.dtype, d.device = 0, 1, 1, _lib.QDAS_F32, -1
    d.fs, d.fsr, d.cinv = 1.0, 1.0, 1.0
    _rejects(L.qdas_greens(C.byref(d), BUF, None), b"greens: element subdivisions must be >= 1")


def test_pre_plan_create_rejects_an_unknown_input_type():
    L = _lib.lib()
    d = _lib.PreDesc()
    d.T, d.K, d.in_type, d.device, d.fs = 64, 4, 2, -1, 1.0
    out = C.c_void_p(1)
    _rejects(L.qdas_pre_plan_create(C.byref(out), C.byref(d)), b"pre: input type must be fp32 or int16")
    assert out.value is None          # the handle is cleared before anything is checked


def test_shift_sum_rejects_flag_bits_above_the_interpolator():
    L = _lib.lib()
    d = _lib.ShiftDesc()
    d.T, d.To, d.N, d.M, d.Mo, d.F = 16, 16, 2, 2, 2, 1
    d.flag, d.dtype, d.cplx, d.device = 8, _lib.QDAS_F32, 1, -1
    _rejects(L.qdas_shift_sum(C.byref(d), BUF, BUF, None), b"Interp option not recognized: 8")


def test_convd_rejects_an_unknown_shape_and_unknown_broadcast_bits():
    L = _lib.lib()
    d = _lib.ConvdDesc()
    d.C, d.M, d.N, d.S, d.dtype, d.cplx, d.shape, d.bcast, d.device = 1, 16, 4, 1, _lib.QDAS_F32, 1, 4, 0, -1
    _rejects(L.qdas_convd(C.byref(d), BUF, BUF, BUF, None), b"convd: shape must be one of {'full', 'same', 'valid'}")
    d.shape, d.bcast = _lib.QDAS_CONV_FULL, 16
    _rejects(L.qdas_convd(C.byref(d), BUF, BUF, BUF, None), b"convd: unknown broadcast bits")


def test_convd_len():
    L = _lib.lib()
    full, same, valid, causal = _lib.QDAS_CONV_FULL, _lib.QDAS_CONV_SAME, _lib.QDAS_CONV_VALID, _lib.QDAS_CONV_CAUSAL
    assert [L.qdas_convd_len(10, 4, s) for s in (full, same, valid, causal)] == [13, 10, 7, 10]
    assert [L.qdas_convd_len(3, 5, s) for s in (full, same, valid, causal)] == [7, 3, 0, 3]          # M < N: 'valid' is empty
    assert L.qdas_convd_len(5, 5, valid) == 1
    assert L.qdas_convd_len(0, 4, full) == 0 and L.qdas_convd_len(4, 0, same) == 0 and L.qdas_convd_len(10, 4, 4) == 0


def test_permute3_rejects_a_three_byte_element():
    L = _lib.lib()
    _rejects(L.qdas_permute3(BUF, BUF, 4, 3, 2, 3, None), b"permute3: element size must be 2, 4, 8 or 16 bytes")


def test_device_copy_rejects_an_unknown_kind():
    L = _lib.lib()
    _rejects(L.qdas_device_copy(BUF, BUF, 16, 3, -1), b"qdas_device_copy: null pointer or unknown kind")


def test_every_function_of_the_header_is_an_unmangled_dynamic_symbol():
    """an `extern "C"` lost when an entry moves between files leaves a mangled symbol: the loader of a C caller does not find it"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    so = os.path.join(ROOT, "qups_amd", "libqdas.so")
    if not os.path.exists(so) or not os.path.exists(kernel_regs.READELF):
        pytest.skip("libqdas.so / llvm-readelf not available")
    header = open(os.path.join(ROOT, "include", "qdas.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)          # (comments name functions of the reference with the same prefix)
    declared = set(re.findall(r"\b(qdas_\w+)\s*\(", header))
    assert len(declared) >= len(_lib.SYMBOLS) and set(_lib.SYMBOLS) <= declared
    out = subprocess.run([kernel_regs.READELF, "--dyn-syms", "-W", so], capture_output=True, text=True, check=True).stdout
    defined = set()
    for line in out.splitlines():
        f = line.split()          # Num: Value Size Type Bind Vis Ndx Name
        if len(f) == 8 and f[3] == "FUNC" and f[4] in ("GLOBAL", "WEAK") and f[6] != "UND":
            defined.add(f[7].split("@")[0])
    assert not sorted(declared - defined), sorted(declared - defined)
