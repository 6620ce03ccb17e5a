"""The 'wbilerp' and 'rayintegrals' commands of mex/qdas_mex.c, driven over the fake MEX runtime (tests/fake_mex/) and the real libqdas.so by
tests/fake_mex/run_raypaths.c, which compares every result bit for bit with the C ABI called directly (the indices 1-based, 0 = empty)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_mex")
SRC = os.path.join(ROOT, "mex", "qdas_mex.c")
CFLAGS = ["-std=c99", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-I", os.path.join(ROOT, "include"), "-I", FAKE]


def test_gateway_and_raypaths_driver_link(tmp_path):
    """without a device: the gateway, the fake runtime and the driver compile and link against the library"""
    exe = str(tmp_path / "run_raypaths")
    lib = os.path.join(ROOT, "qups_amd")
    cmd = ["gcc", "-O1", *CFLAGS, SRC, os.path.join(FAKE, "fake_mex_runtime.c"), os.path.join(FAKE, "run_raypaths.c"),
           "-L", lib, "-lqdas", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.gpu
def test_raypaths_commands_match_the_c_abi(tmp_path):
    exe = str(tmp_path / "run_raypaths")
    lib = os.path.join(ROOT, "qups_amd")
    cmd = ["gcc", "-O1", *CFLAGS, SRC, os.path.join(FAKE, "fake_mex_runtime.c"), os.path.join(FAKE, "run_raypaths.c"),
           "-L", lib, "-lqdas", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "raypaths gateway OK" in r.stdout, r.stdout + r.stderr
    assert "bit-identical to the C ABI" in r.stdout
