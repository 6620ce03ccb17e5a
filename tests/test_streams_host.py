"""The census behind tests/test_gpu_streams.py, on the CPU: every prototype of include/qdas.h that takes a ``void *stream`` maps to a stream case of that
file's table, or to an exemption with a reason.  A new entry without a stream case fails here, without a GPU."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the entries that take a stream today (a change of this list is a change of the ABI: it shows in the diff)
KNOWN = """
qdas_plan_execute           qdas_plan_execute_frames    qdas_plan_delays
qdas_fold                   qdas_plan_execute_sharded   qdas_DAS
qdas_DASf                   qdas_DASh                   qdas_delays
qdas_delaysf                qdas_das_lut                qdas_wsinterpd
qdas_greens                 qdas_shift_sum              qdas_convd
qdas_iir                    qdas_coherence              qdas_eikonal
qdas_eikonal_tables         qdas_adjoint                qdas_migration
qdas_pwznxcorr              qdas_permute3               qdas_pre_execute
""".split()


def stream_entries(text):
    """names of the function prototypes with a ``void *stream`` parameter, comments stripped"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    names = []
    for m in re.finditer(r"\b(qdas_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
            names.append(m.group(1))
    return names


def _header():
    with open(os.path.join(ROOT, "include", "qdas.h")) as f:
        return f.read()


def test_the_parser_reads_prototypes_not_comments():
    text = """/* int qdas_ghost(void *stream); */
    // int qdas_ghost2(void *stream);
    int  qdas_a(const qdas_desc *d, const void *x,
                void *y, void *stream);
    int qdas_b(qdas_plan *p, uint64_t F);       /* asynchronous on `stream` */
    typedef struct { void *stream; } not_a_function;
    int qdas_c (void * stream);"""
    assert stream_entries(text) == ["qdas_a", "qdas_c"]


def test_the_header_has_the_entries_we_know():
    got = stream_entries(_header())
    assert len(got) == len(set(got))
    assert sorted(got) == sorted(KNOWN), (sorted(set(got) - set(KNOWN)), sorted(set(KNOWN) - set(got)))


def test_every_entry_with_a_stream_has_a_stream_case():
    from tests import test_gpu_streams as S
    missing = []
    for name in stream_entries(_header()):
        ids = S.HEADER.get(name, [])
        reason = S.EXEMPT.get(name)
        if reason:
            assert isinstance(reason, str) and len(reason.split()) >= 4, f"{name}: an exemption needs a reason"
            continue
        if not ids or any(i not in S.CASES for i in ids):
            missing.append((name, [i for i in ids if i not in S.CASES]))
    assert not missing, f"entries of include/qdas.h that take a stream and have no case in tests/test_gpu_streams.py (or name a case that does not exist): {missing}"
    stale = sorted((set(S.HEADER) | set(S.EXEMPT)) - set(stream_entries(_header())))
    assert not stale, f"tests/test_gpu_streams.py maps entries the header does not have: {stale}"


def test_every_blocking_entry_is_cited_and_used():
    """BLOCKS = {entry: "file:line reason"}: every key is the entry of a case (or of one of the further tests), every value names a file of the repository"""
    from tests import test_gpu_streams as S
    entries = {e for e, _, _, _ in S.CASES.values()} | {"plan_close"}
    for name, why in S.BLOCKS.items():
        assert name in entries, f"BLOCKS lists '{name}', which no case belongs to"
        path = why.split(" -- ")[0].split(":")[0]
        assert " -- " in why and os.path.exists(os.path.join(ROOT, path)), (name, why)
