"""The 'raybackproject' command of mex/qdas_mex.c, driven over the fake MEX runtime (tests/fake_mex/) and the real libqdas.so by
tests/fake_mex/run_raybackproject.c, which compares every result bit for bit with the C ABI called directly; the double case is then held against the Python
layer on the same data."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_mex")
SRC = os.path.join(ROOT, "mex", "qdas_mex.c")
CFLAGS = ["-std=c99", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-I", os.path.join(ROOT, "include"), "-I", FAKE]


def _build(tmp_path):
    exe = str(tmp_path / "run_raybackproject")
    lib = os.path.join(ROOT, "qups_amd")
    cmd = ["gcc", "-O1", *CFLAGS, SRC, os.path.join(FAKE, "fake_mex_runtime.c"), os.path.join(FAKE, "run_raybackproject.c"),
           "-L", lib, "-lqdas", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_gateway_and_raybackproject_driver_link(tmp_path):
    """without a device: the gateway, the fake runtime and the driver compile (warnings are errors) and link against the library; the command is wired in"""
    _build(tmp_path)
    text = open(SRC).read()
    assert "'raybackproject'" in text and "qdas_raypaths_backproject(" in text and 'strcmp(cmd, "raybackproject")' in text


@pytest.mark.gpu
def test_raybackproject_command_matches_the_c_abi_and_the_python_layer(tmp_path):
    import torch
    from qups_amd import raypaths as RP
    exe = _build(tmp_path)
    dump = str(tmp_path / "double.bin")
    r = subprocess.run([exe, dump], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "raybackproject gateway OK" in r.stdout, r.stdout + r.stderr
    assert "bit-identical to the C ABI" in r.stdout
    # the driver's double case: X = 11, Z = 9, J = 6, F = 2, strides [Z 1] -- an X x Z array in row-major terms, ord = "XZ"
    X, Z, J, F = 11, 9, 6, 2
    raw = np.fromfile(dump, np.float64)
    assert raw.size == J * F + X * Z * F + X * Z
    rr, g, col = raw[:J * F].reshape(F, J), raw[J * F:J * F + X * Z * F].reshape(F, X, Z), raw[J * F + X * Z * F:].reshape(X, Z)
    pa = np.array([[-4, 1], [5, -4], [-7, 0], [2, 2], [np.nan, 0], [-4.5, 3.25]]).T
    pb = np.array([[3, -2], [5, 4], [-6, 3], [2, 2], [1, 1], [4.75, -3.5]]).T
    gp, cp = RP.ray_backproject(torch.from_numpy(rr).cuda(), np.arange(-5.0, 6.0), np.arange(-4.0, 5.0), pa, pb, ord="XZ", colsum=True)
    assert np.array_equal(gp.cpu().numpy(), g) and np.array_equal(cp.cpu().numpy(), col) and col.sum() > 0
