"""The 'msfm3d' command of mex/qdas_mex.c, driven over the fake MEX runtime (tests/fake_mex/) and the real libqdas.so by tests/fake_mex/run_eikonal3.c,
which compares every result bit for bit with qdas_eikonal3 called directly; one of its maps is also compared with ``qups_amd.msfm3d``."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_mex")
SRC = os.path.join(ROOT, "mex", "qdas_mex.c")
CFLAGS = ["-std=c99", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-I", os.path.join(ROOT, "include"), "-I", FAKE]


def test_gateway_and_eikonal3_driver_compile(tmp_path):
    for src in (SRC, os.path.join(FAKE, "run_eikonal3.c")):
        r = subprocess.run(["gcc", "-c", *CFLAGS, src, "-o", str(tmp_path / (os.path.basename(src) + ".o"))], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    assert "'msfm3d'" in open(SRC).read() and "qdas_eikonal3(" in open(SRC).read() and "qdas_eikonal3_work_bytes(" in open(SRC).read()


def test_gateway_links_against_the_library(tmp_path):
    """every symbol the gateway and the driver use is exported (no device is needed to link)"""
    exe = str(tmp_path / "run_eikonal3")
    lib = os.path.join(ROOT, "qups_amd")
    r = subprocess.run(["gcc", "-O1", *CFLAGS, SRC, os.path.join(FAKE, "fake_mex_runtime.c"), os.path.join(FAKE, "run_eikonal3.c"),
                        "-L", lib, "-lqdas", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.gpu
def test_msfm3d_command_matches_the_c_abi_and_the_python_entry(tmp_path):
    exe = str(tmp_path / "run_eikonal3")
    lib = os.path.join(ROOT, "qups_amd")
    cmd = ["gcc", "-O1", *CFLAGS, SRC, os.path.join(FAKE, "fake_mex_runtime.c"), os.path.join(FAKE, "run_eikonal3.c"),
           "-L", lib, "-lqdas", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, str(tmp_path / "map.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "eikonal3 gateway OK" in r.stdout, r.stdout + r.stderr
    assert "bit-identical to the C ABI" in r.stdout
    # the gateway's map of the two-point set {1:2} against msfm3d on the driver's volume
    import numpy as np
    from qups_amd import msfm3d
    i, j, l = np.meshgrid(np.arange(19), np.arange(13), np.arange(10), indexing="ij")
    F = np.where(i < 6, 6.0e6, np.where(i < 12, 5.6e6, 6.4e6)) + 1.0e5 * ((i * 7 + j * 3 + l * 5) % 5)
    T = msfm3d(F, np.array([[1.0, 19.0], [1.0, 13.0], [1.0, 10.0]])).cpu().numpy()
    got = np.fromfile(str(tmp_path / "map.bin"), np.float64).reshape((19, 13, 10), order="F")
    assert np.array_equal(got, T)
