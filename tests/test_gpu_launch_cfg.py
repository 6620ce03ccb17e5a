"""Which launch configuration of the fused kernel (``csrc/das_tile_cfg.h``) every reachable family of plans REALLY launches, read from the kernel census
(``QDAS_KERNEL_CENSUS``) of one tiny plan per family, and each family's image against the same plan forced to the generic kernel.

The expected (configuration, probe) pairs were recorded from the build BEFORE the configurations moved into one table and one selector, and are literals:
the selector, the launcher's table of instantiations and ``launch_legal``'s ``cfg`` must go on naming the same kernels.  Configurations 9 (frames beyond
2 GiB) and 14 (tiles that misfit 192-sample windows) are not forced at these sizes: ``tests/test_launch_cfg.py`` and the rest of the suite cover them."""
import json
import os
import subprocess
import sys

import pytest

from tests.test_gpu_parity import TOL32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the bounds tests/test_gpu_parity.py states for each precision (its module docstring; TOL32 is its constant, the generic kernel's bound for fp32 data)
TOL16 = 2e-3
TOL64 = 1e-10

# family -> the census lines it adds, as (configuration, probe).  One process: an instantiation is listed once, so the probes of "2-frame stream" and
# "4-frame stream" (the probe kernels of "fp32 general" and "BF") do not show again.
EXPECTED = {
    "fp32 general":             ([(0, 0), (0, 1)], TOL32),
    "fp16 general":             ([(2, 0), (2, 1)], TOL16),
    "fp64":                     ([(13, 0), (13, 1)], TOL64),
    "BF":                       ([(0, 1), (12, 0)], TOL32),
    "table-driven fp32":        ([(10, 0), (10, 1)], TOL32),
    "folded":                   ([(19, 0), (19, 1)], TOL32),
    "folded, lateral mirror":   ([(17, 0), (17, 1)], TOL32),
    "general, lateral mirror":  ([(0, 1), (3, 0)], TOL32),
    "fp16 reciprocal, no fold": ([(8, 0), (8, 1)], TOL16),
    "2-frame stream":           ([(3, 0)], TOL32),
    "4-frame stream":           ([(0, 0), (3, 0), (5, 0)], TOL32),       # (a stream resolves the kernels of its shorter tails too)
    "2-frame folded stream":    ([(19, 0), (19, 1), (21, 0)], TOL32),
}


def test_every_family_launches_its_configuration_and_matches_the_generic_kernel(tmp_path):
    env = dict(os.environ, QDAS_KERNEL_CENSUS=str(tmp_path / "census.txt"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "launch_cfg_child.py")], env=env, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    for name, got in res.items():
        print(f"{name:26s} census {got['census']}  |tiled - generic| / max {got['err']:.3e}")
    assert list(res) == list(EXPECTED)
    for name, (pairs, tol) in EXPECTED.items():
        assert [tuple(p) for p in res[name]["census"]] == pairs, (name, res[name]["census"])
        assert res[name]["err"] <= tol, (name, res[name]["err"], tol)
