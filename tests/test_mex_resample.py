"""The 'resample' command of mex/qdas_mex.c, driven over the fake MEX runtime (tests/fake_mex/) and the real libqdas.so by tests/fake_mex/run_resample.c,
which compares every result bit for bit with the C ABI called directly and writes them to a file; here the same data go through the Python layer
(``qups_amd.resample``) and must give the same bits."""
import importlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_mex")
SRC = os.path.join(ROOT, "mex", "qdas_mex.c")
CFLAGS = ["-std=c99", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-I", os.path.join(ROOT, "include"), "-I", FAKE]
NT, NC, NK = 301, 3, 41


def build_gateway(tmp_path=None):
    import tempfile
    exe = os.path.join(str(tmp_path) if tmp_path is not None else tempfile.mkdtemp(prefix="qdas_mex_resample_"), "run_resample")
    lib = os.path.join(ROOT, "qups_amd")
    cmd = ["gcc", "-O1", *CFLAGS, SRC, os.path.join(FAKE, "fake_mex_runtime.c"), os.path.join(FAKE, "run_resample.c"),
           "-L", lib, "-lqdas", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_gateway_and_resample_driver_link(tmp_path):
    """without a device: the gateway, the fake runtime and the driver compile (-Wall -Wextra -Werror) and link against the library"""
    build_gateway(tmp_path)
    text = open(SRC).read()
    assert "'resample'" in text and "qdas_resample(" in text


def driver_data(kind, cplx):
    """the sequence tests/fake_mex/run_resample.c forms: T x C, time fastest in the driver -- here as a T x C array"""
    i = np.arange(NT * NC, dtype=np.int64)
    s = lambda j: ((j * 7919 + 13) % 2001 - 1000).astype(np.float64)
    v = s(i) + (1j * s(i + 5) if cplx else 0)
    if kind == "i16":
        x = v.astype(np.int16)
    else:
        rt = np.float32 if kind == "f32" else np.float64
        x = (v.real / 256.0).astype(rt) + (1j * (v.imag / 256.0).astype(rt) if cplx else 0)
        x = x.astype({(np.float32, 0): np.float32, (np.float32, 1): np.complex64, (np.float64, 0): np.float64, (np.float64, 1): np.complex128}[(rt, cplx)])
    return x.reshape(NC, NT).T


@pytest.mark.gpu
def test_resample_command_matches_the_c_abi_and_the_python_layer(tmp_path):
    import torch
    RS = importlib.import_module("qups_amd.resample")
    dump = str(tmp_path / "resample.bin")
    r = subprocess.run([build_gateway(tmp_path), dump], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "resample gateway OK" in r.stdout, r.stdout + r.stderr
    assert "bit-identical to the C ABI" in r.stdout
    raw = open(dump, "rb").read()
    h = ((np.arange(NK) * 31 + 7) % 17 - 8) / 64.0
    at = 0
    for kind, cplx in (("i16", 0), ("f32", 0), ("f32", 1), ("f64", 0), ("f64", 1)):
        odt = {("i16", 0): np.float32, ("f32", 0): np.float32, ("f32", 1): np.complex64, ("f64", 0): np.float64, ("f64", 1): np.complex128}[(kind, cplx)]
        x = torch.from_numpy(np.ascontiguousarray(driver_data(kind, cplx))).cuda()
        for p, q, edge in ((5, 4, "zero"), (1, 1, "odd")):
            J = RS.resample_len(NT, p, q)
            nbytes = J * NC * np.dtype(odt).itemsize
            mex = np.frombuffer(raw[at:at + nbytes], odt).reshape(NC, J).T
            at += nbytes
            got = (RS.resample(x, p, q, h=h) if edge == "zero" else RS.polyphase(h, x, 1, 1, (NK - 1) // 2, NT, edge="odd")).cpu().numpy()
            assert got.shape == mex.shape and got.dtype == mex.dtype
            assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(mex).view(np.uint8)), (kind, cplx, p, q)
    assert at == len(raw)
