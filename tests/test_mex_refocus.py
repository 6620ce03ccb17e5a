"""The 'refocus' command of mex/qdas_mex.c, driven over the fake MEX runtime (tests/fake_mex/) and the real libqdas.so by
tests/fake_mex/run_refocus.c, which compares every result bit for bit with qdas_refocus called directly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_mex")
SRC = os.path.join(ROOT, "mex", "qdas_mex.c")
CFLAGS = ["-std=c99", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-I", os.path.join(ROOT, "include"), "-I", FAKE]


def test_gateway_and_refocus_driver_compile(tmp_path):
    for src in (SRC, os.path.join(FAKE, "run_refocus.c")):
        r = subprocess.run(["gcc", "-c", *CFLAGS, src, "-o", str(tmp_path / (os.path.basename(src) + ".o"))], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    text = open(SRC).read()
    assert "'refocus'" in text and "qdas_refocus(" in text and "qdas_refocus_work_bytes(" in text


@pytest.mark.gpu
def test_refocus_command_matches_the_c_abi(tmp_path):
    exe = str(tmp_path / "run_refocus")
    lib = os.path.join(ROOT, "qups_amd")
    cmd = ["gcc", "-O1", *CFLAGS, SRC, os.path.join(FAKE, "fake_mex_runtime.c"), os.path.join(FAKE, "run_refocus.c"),
           "-L", lib, "-lqdas", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "refocus gateway OK" in r.stdout, r.stdout + r.stderr
    assert "bit-identical to the C ABI" in r.stdout
