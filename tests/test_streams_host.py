"""Host side (no GPU) of the stream-contract tests: every exported function of include/vae_step.h that takes a vae_stream_t is
either called by a case of tests/test_streams_gpu.py or listed in its NOT_COVERED with a reason, so a new entry point cannot
be added without deciding where it stands.  The case table is collected by importing the module, which touches no GPU."""
import inspect
import os
import re

from tests import test_streams_gpu as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vae_step.h")


def stream_entry_points():
    """Names of the functions declared in the header with a vae_stream_t parameter (comments removed first)."""
    hdr = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    found = [m.group(1) for m in re.finditer(r"\b(vae_\w+)\s*\(([^;{}]*?)\)\s*;", hdr) if re.search(r"\bvae_stream_t\b", m.group(2))]
    assert len(found) == len(set(found))
    return found


def covered():
    names = set()
    for c in cases.CASES + cases.PY_CASES:
        names |= set(c.covers)
    return names


def test_header_parse_finds_the_stream_functions():
    names = stream_entry_points()
    assert len(names) >= 37, names
    assert {"vae_forward", "vae_comm_stream", "vae_selftest_tr16", "vae_nearest_rolls", "vae_train_step_fused_clipped"} <= set(names)
    assert "vae_set_option" not in names and "vae_create" not in names


def test_every_stream_entry_point_is_covered_or_excused():
    names, cov = stream_entry_points(), covered()
    undecided = [n for n in names if n not in cov and n not in cases.NOT_COVERED]
    assert not undecided, f"entry points with a stream argument that no case calls and NOT_COVERED does not name: {undecided}"
    both = [n for n in cases.NOT_COVERED if n in cov]
    assert not both, both
    stale = [n for n in list(cases.NOT_COVERED) + sorted(cov) if n not in names]
    assert not stale, f"not functions with a stream argument (any more): {stale}"


def test_tables_carry_reasons():
    for table in (cases.NOT_COVERED, cases.EXEMPT):
        for name, reason in table.items():
            assert isinstance(reason, str) and len(reason.split()) >= 5, (name, reason)
    assert set(cases.NOT_COVERED) == {"vae_selftest_tr16", "vae_broadcast_state"}
    for c in cases.CASES + cases.PY_CASES:
        assert c.reads_back is None or (not c.sync_free and len(c.reads_back.split()) >= 5), c.name


def test_a_covered_entry_point_is_really_called():
    """`covers` is a claim: each C-ABI case's names are calls in the module's own source, and every case of the C-ABI table holds
    the host to `pending` (the Python-level cases call through the package)."""
    src = inspect.getsource(cases)
    called = set(re.findall(r"lib\(\)\.(vae_\w+)\(|L_\.(vae_\w+)\(", src))
    called = {a or b for a, b in called}
    for c in cases.CASES:
        assert c.sync_free and c.reads_back is None, c.name
        missing = [n for n in c.covers if n not in called]
        assert not missing, (c.name, missing)
    names = [c.name for c in cases.CASES + cases.PY_CASES]
    assert len(set(names)) == len(names)
