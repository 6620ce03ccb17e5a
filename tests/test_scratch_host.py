"""The census behind tests/test_gpu_scratch.py, on the CPU: the source files that construct a ``Scratch`` (csrc/scratch.hip: the per-stream arena) are exactly
the files that file's ``ARENA_USERS`` table claims to cover, every row it names exists, and DESIGN.md's region table speaks of every one of them.  A new arena
user without a poisoned case fails here, without a GPU."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qups_amd", "csrc")


def scratch_users(text):
    """does the source construct a ``Scratch`` (``Scratch name(stream)``, with or without the namespace)?  Comments stripped."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return re.search(r"\bScratch\s+[A-Za-z_]\w*\s*[({]", text) is not None


def _users():
    out = set()
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))):
        if os.path.basename(path) in ("scratch.hip", "qdas_kernels.h"):          # (the class itself; its debug entry)
            continue
        with open(path) as f:
            if scratch_users(f.read()):
                out.add(os.path.basename(path))
    return out


def test_the_parser_sees_constructions_not_comments():
    assert scratch_users("void f(hipStream_t s) {\n    Scratch scratch(s);   // arena\n}")
    assert scratch_users("qdas::Scratch  ws{s};")
    assert not scratch_users("// Scratch scratch(s);\n/* Scratch a(s); */ int x;")
    assert not scratch_users("class Scratch {\npublic:\n    explicit Scratch(hipStream_t s);\n    Scratch(const Scratch &) = delete;\n    Scratch &operator=(const Scratch &) = delete;\n};")
    assert not scratch_users("void *Scratch::get(size_t bytes) { return nullptr; }  Scratch::~Scratch() {}")


def test_every_arena_user_has_poisoned_cases():
    from tests import test_gpu_scratch as G
    from tests import test_gpu_streams as S
    got, want = _users(), set(G.ARENA_USERS)
    assert got == want, f"files that construct a Scratch without rows in tests/test_gpu_scratch.py ARENA_USERS: {sorted(got - want)}; listed there but no longer users: {sorted(want - got)}"
    for name, ids in G.ARENA_USERS.items():
        assert ids and all(i in S.CASES for i in ids), (name, [i for i in ids if i not in S.CASES])
    assert len(G.WAKE) == len(G.ARENA_USERS) and all(sum(w in ids for ids in G.ARENA_USERS.values()) == 1 for w in G.WAKE)
    assert {next(n for n, ids in G.ARENA_USERS.items() if w in ids) for w in G.WAKE} == want, "the wake test runs one row of every arena user"
    assert len(G.ARENA0_ROWS) == 5 and G.PLAN_ROWS


def test_the_region_table_names_every_arena_user_and_the_switch():
    from tests import test_gpu_scratch as G
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    sec = design[design.index("### 5d."):]
    sec = sec[:sec.index("\n## ")]
    for name in G.ARENA_USERS:
        assert f"`{name}`" in sec, f"DESIGN.md 5d has no region row for csrc/{name}"
    for text, where in ((sec, "DESIGN.md 5d"), (open(os.path.join(ROOT, "include", "qdas.h")).read(), "include/qdas.h")):
        assert "QDAS_SCRATCH_POISON" in text and "QDAS_SCRATCH_ARENA_MAX_MB" in text, where
