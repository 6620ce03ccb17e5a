"""The 'pwznxcorr' command of mex/qdas_mex.c, driven over the fake MEX runtime (tests/fake_mex/) and the real libqdas.so by
tests/fake_mex/run_pwznxcorr.c, which compares every result bit for bit with qdas_pwznxcorr called directly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_mex")
SRC = os.path.join(ROOT, "mex", "qdas_mex.c")
CFLAGS = ["-std=c99", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-I", os.path.join(ROOT, "include"), "-I", FAKE]


def test_pwznxcorr_driver_and_gateway_compile(tmp_path):
    for src in (os.path.join(FAKE, "run_pwznxcorr.c"), SRC):
        r = subprocess.run(["gcc", "-c", *CFLAGS, src, "-o", str(tmp_path / "unit.o")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


@pytest.mark.gpu
def test_pwznxcorr_command_matches_the_c_abi(tmp_path):
    exe = str(tmp_path / "run_pwznxcorr")
    lib = os.path.join(ROOT, "qups_amd")
    cmd = ["gcc", "-O1", *CFLAGS, SRC, os.path.join(FAKE, "fake_mex_runtime.c"), os.path.join(FAKE, "run_pwznxcorr.c"),
           "-L", lib, "-lqdas", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "pwznxcorr gateway OK" in r.stdout, r.stdout + r.stderr
    assert "bit-identical to the C ABI" in r.stdout
