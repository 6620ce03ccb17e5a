"""The launch configurations of the fused kernel WITHOUT a GPU: ``csrc/das_tile_cfg.h`` describes each configuration in one table row and chooses one per
launch in ``select_cfg``.  Both are checked here against literals transcribed from the code they replaced -- the comparisons on the configuration number
that ``launch_tile_i`` and ``jit.hip`` spelled out, the launcher's nested ternary over fifteen per-configuration files and the folded family's sub-dispatch --
not against themselves."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qups_amd", "csrc")

# ---- what each number meant, as the old comparisons spelled it
FOLD = {17, 18, 19, 20, 21}
MIRQ = {15, 16, 17, 18, 20}
SYM = {1, 7, 8} | MIRQ | FOLD
FB2 = {3, 4, 20, 21}
FB4 = {5, 6}
BIG, LUT, BFM = {9}, {10, 11}, {12}
BYTES4, BYTES16 = {2, 4, 6, 8, 11, 16}, {13}
HIPRTC_ONLY = {1, 7, 15}
STAGE = [(16, 32, 192), (16, 16, 192), (16, 32, 384), (16, 16, 192), (16, 16, 384), (16, 8, 192), (16, 8, 384), (16, 16, 128), (16, 16, 256), (16, 32, 192), (16, 32, 192),
         (16, 32, 384), (16, 32, 192), (16, 16, 192), (16, 16, 384), (16, 16, 128), (16, 16, 256), (16, 32, 128), (16, 16, 192), (16, 32, 192), (16, 16, 128), (16, 16, 192)]

# ---- the launcher's choice, one line per row of the rule table (first match first); -1: no configuration.  Arguments of select_cfg:
#      dtype (0 fp64, 1 fp32, 2 fp16), sym, nf, narrow, mirq, fold, big, lut, bf, probe
SELECT = [
    ((0, 0, 1, 0, 0, 0, 0, 0, 0, 0), 13), ((0, 0, 1, 0, 0, 0, 0, 0, 0, 1), 13),                    # fp64, launch and probe
    ((1, 1, 1, 1, 0, 1, 0, 0, 0, 1), 17), ((1, 1, 1, 0, 0, 1, 0, 0, 0, 1), 19),                    # folded: probes with 128- / 192-sample windows
    ((1, 1, 1, 1, 0, 0, 0, 0, 0, 1), 17), ((1, 1, 1, 0, 0, 0, 0, 0, 0, 1), 19),                    # ... the probes of an UNFOLDED fp32 reciprocal plan run the same rows
    ((1, 1, 2, 1, 1, 1, 0, 0, 0, 0), 20), ((1, 1, 2, 0, 1, 1, 0, 0, 0, 0), -1),                    # folded, two frames, mirror: narrow windows only
    ((1, 1, 2, 0, 0, 1, 0, 0, 0, 0), 21), ((1, 1, 2, 1, 0, 1, 0, 0, 0, 0), 21),                    # folded, two frames
    ((1, 1, 4, 0, 0, 1, 0, 0, 0, 0), -1), ((1, 1, 3, 1, 1, 1, 0, 0, 0, 0), -1),                    # folded, more than two frames
    ((1, 1, 1, 0, 0, 1, 0, 0, 0, 0), 19), ((1, 1, 1, 1, 0, 1, 0, 0, 0, 0), 19),                    # folded, no mirror
    ((1, 1, 1, 1, 1, 1, 0, 0, 0, 0), 17), ((1, 1, 1, 0, 1, 1, 0, 0, 0, 0), 18),                    # folded, mirror: narrow / 192-sample windows
    ((1, 0, 1, 0, 0, 0, 0, 1, 0, 0), 10), ((2, 0, 1, 0, 0, 0, 0, 1, 0, 0), 11),                    # table-driven delays
    ((1, 0, 1, 0, 0, 0, 0, 1, 0, 1), 10), ((2, 0, 1, 0, 0, 0, 0, 1, 0, 1), 11),                    # ... their probes too
    ((1, 0, 2, 0, 0, 0, 0, 1, 0, 0), 10),                                                          # ... a hiprtc mirror build's launch: still the table rows
    ((2, 1, 1, 0, 1, 0, 0, 0, 0, 0), 16),                                                          # mirq and fp16
    ((2, 1, 1, 0, 0, 0, 0, 0, 0, 0), 8), ((2, 1, 1, 0, 0, 0, 0, 0, 0, 1), 8),                      # sym and fp16 (its probe: mirq is 0)
    ((1, 1, 1, 0, 0, 0, 0, 0, 0, 0), 1), ((1, 1, 1, 1, 0, 0, 0, 0, 0, 0), 7), ((1, 1, 1, 1, 1, 0, 0, 0, 0, 0), 15),      # sym otherwise: rows without a translation unit
    ((1, 0, 4, 0, 0, 0, 0, 0, 0, 0), 5), ((2, 0, 4, 0, 0, 0, 0, 0, 0, 0), 6),                      # four frames
    ((1, 0, 2, 0, 0, 0, 0, 0, 0, 0), 3), ((2, 0, 2, 0, 0, 0, 0, 0, 0, 0), 4),                      # two frames / a general-mode lateral-mirror plan's one frame
    ((2, 0, 1, 0, 0, 0, 0, 0, 0, 0), 2), ((2, 0, 1, 0, 0, 0, 0, 0, 0, 1), 2), ((2, 0, 1, 2, 0, 0, 0, 0, 0, 0), 2),      # fp16 (before the 384-sample rule)
    ((1, 0, 1, 2, 0, 0, 0, 0, 0, 0), 14), ((1, 0, 1, 2, 0, 0, 0, 0, 0, 1), 14),                    # narrow == 2
    ((1, 0, 1, 0, 0, 0, 0, 0, 1, 0), 12), ((1, 0, 1, 0, 0, 0, 0, 0, 1, 1), 0),                     # 'BF': probes with configuration 0
    ((1, 0, 1, 0, 0, 0, 1, 0, 0, 0), 9), ((1, 0, 1, 0, 0, 0, 1, 0, 0, 1), 0),                      # re-basing: probes with configuration 0
    ((1, 0, 1, 0, 0, 0, 0, 0, 0, 0), 0), ((1, 0, 1, 0, 0, 0, 0, 0, 0, 1), 0),                      # otherwise
    ((1, 0, 2, 0, 0, 0, 1, 0, 1, 0), 3),                                                           # (two frames before 'BF' / re-basing: launch_legal refuses those)
]

PROGRAM = r"""
#include <cstdio>
#include "das_tile_cfg.h"
using namespace qdas;
static_assert(select_cfg(1, 1, 1, 1, 1, 1) == 17, "the selector is usable in constant expressions");
int main() {
    printf("ncfg %d\n", NCFG);
    for (int c = 0; c < NCFG; ++c) {
        const Cfg &g = CFGS[c];
        printf("row %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", c, g.waves, g.mb, g.w, g.nbuf, g.psz, g.bpc, g.bytes, g.frames, (int)g.sym, (int)g.mirq, (int)g.fold, (int)g.big,
               (int)g.lut, (int)g.bfm, (int)g.tu);
    }
    int a[10];
    while (scanf("%d %d %d %d %d %d %d %d %d %d", a, a + 1, a + 2, a + 3, a + 4, a + 5, a + 6, a + 7, a + 8, a + 9) == 10)
        printf("sel %d\n", select_cfg(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9]));
    return 0;
}
"""


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """rows of CFGS and select_cfg over SELECT, through a g++ program (no HIP): the header stays usable by the GPU-less mode tests"""
    d = tmp_path_factory.mktemp("launch_cfg")
    src, exe = d / "cfg_dump.cpp", d / "cfg_dump"
    src.write_text(PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], input="".join(" ".join(map(str, k)) + "\n" for k, _ in SELECT), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    rows = {int(p[1]): tuple(int(v) for v in p[2:]) for p in (ln.split() for ln in r.stdout.splitlines()) if p[0] == "row"}
    sel = [int(ln.split()[1]) for ln in r.stdout.splitlines() if ln.startswith("sel ")]
    assert int(r.stdout.split()[1]) == 22 and sorted(rows) == list(range(22)) and len(sel) == len(SELECT)
    return rows, sel


def test_every_row_of_the_table_says_what_the_old_comparisons_said(table):
    rows, _ = table
    for c, (waves, mb, w, nbuf, psz, bpc, nbytes, frames, sym, mirq, fold, big, lut, bfm, tu) in rows.items():
        assert (waves, mb, w) == STAGE[c] and (nbuf, psz, bpc) == (2, 16, 1), c
        assert nbytes == (4 if c in BYTES4 else 16 if c in BYTES16 else 8), c
        assert frames == (2 if c in FB2 else 4 if c in FB4 else 1), c
        assert (sym, mirq, fold, big, lut, bfm) == tuple(int(c in s) for s in (SYM, MIRQ, FOLD, BIG, LUT, BFM)), c
        assert tu == int(c not in HIPRTC_ONLY), c


def test_the_selector_follows_the_rule_table(table):
    _, sel = table
    got = {k: s for (k, _), s in zip(SELECT, sel)}
    assert got == dict(SELECT), {k: (got[k], want) for k, want in SELECT if got[k] != want}
    assert {want for _, want in SELECT} >= set(range(22)) | {-1}          # every configuration, and "none", is some rule's answer


def test_the_makefile_builds_one_object_per_row_with_a_translation_unit():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    cfgs = [int(v) for v in re.search(r"^TILE_CFGS = (.*)$", mk, re.M).group(1).split()]
    assert cfgs == sorted(set(range(22)) - HIPRTC_ONLY)


def _lib():
    from qups_amd import _lib
    return _lib.lib()


def test_variant_prebuilt_answers_what_the_old_comparisons_answered():
    """qdas_kernel_variant_prebuilt over all 22 x 6 x 2 x 2 arguments (and the numbers around them): -1 exactly where the old literals said so, else
    qdas_debug_tile_prebuilt's bit"""
    L = _lib()
    for cfg in range(-1, 24):
        for interp in range(-1, 7):
            for fm in (0, 1):
                for wt in (0, 1):
                    known = cfg == 0 or 2 <= cfg <= 6 or 8 <= cfg <= 14 or 16 <= cfg <= 21
                    if not known or interp < 0 or interp > 5 or interp == 4 or (cfg >= 17 and wt) or (cfg == 5 and (fm or wt)):
                        want = -1
                    else:
                        want = L.qdas_debug_tile_prebuilt(cfg, interp, fm, wt, 0)
                    assert L.qdas_kernel_variant_prebuilt(cfg, interp, fm, wt) == want, (cfg, interp, fm, wt)


def test_warm_configs_are_the_configurations_the_library_knows():
    from qups_amd import warm
    L = _lib()
    known = tuple(c for c in range(22) if any(L.qdas_kernel_variant_prebuilt(c, i, 0, 0) != -1 for i in range(6)))
    assert warm.CONFIGS == known
