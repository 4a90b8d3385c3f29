"""The option table of vae_set_option, host side (no GPU): the library's own list (vae_option_info) against the names the
tests, tools and bench.py pass, and against the documentation at vae_set_option in include/vae_step.h."""
import ctypes
import glob
import os
import re

from torch_vae_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vae_step.h")
OPTION = r"(?:use|knob)_[a-z0-9_]+"


def option_table():
    """{name: default} in table order, enumerated to the end."""
    L, table, i = _lib.lib(), [], 0
    name, default = ctypes.c_char_p(), ctypes.c_int()
    while L.vae_option_info(i, ctypes.byref(name), ctypes.byref(default)) == 0:
        table.append((name.value.decode(), default.value))
        i += 1
        assert i < 1000
    assert L.vae_option_info(i, ctypes.byref(name), ctypes.byref(default)) == -1      # one past the end (and the loop's exit)
    assert L.vae_option_info(i + 1, ctypes.byref(name), ctypes.byref(default)) == -1
    assert L.vae_option_info(-1, ctypes.byref(name), ctypes.byref(default)) == -1
    return table


def documented_options():
    """[(name, default)] of every `name [n]` token in the comment in front of vae_set_option's declaration."""
    hdr = open(HEADER).read()
    end = hdr.index("int vae_set_option(")
    start = hdr.rindex("/*", 0, end)
    return [(m.group(1), int(m.group(2))) for m in re.finditer(r"\b(" + OPTION + r") \[(-?\d+)\]", hdr[start:end])]


def names_passed_by_callers():
    """Option names that tests/, tools/ and bench.py hand to vae_set_option: byte literals next to a vae_set_option call, the
    KNOB=VALUE pairs of bench.py's --set, and the keys of option dicts."""
    files = [os.path.join(ROOT, "bench.py")]
    for d in ("tests", "tools"):
        files += [f for f in glob.glob(os.path.join(ROOT, d, "**", "*"), recursive=True) if f.endswith((".py", ".sh"))]
    found = {}
    for f in files:
        if os.path.abspath(f) == os.path.abspath(__file__):
            continue
        text = open(f).read()
        for pat in (r"vae_set_option\([^\n]*?b\"(" + OPTION + r")\"", r"--set[ =](" + OPTION + r")=", r"[\"'](" + OPTION + r")[\"']\s*:\s*-?\d",
                    r"\(\s*[\"'](" + OPTION + r")[\"']\s*,\s*-?\d"):
            for m in re.finditer(pat, text):
                found.setdefault(m.group(1), os.path.relpath(f, ROOT))
    return found


def test_option_names_are_unique():
    names = [n for n, _ in option_table()]
    assert len(names) > 40 and len(set(names)) == len(names)
    assert all(re.fullmatch(OPTION, n) for n in names)


def test_every_option_a_caller_passes_is_in_the_table():
    table = dict(option_table())
    passed = names_passed_by_callers()
    assert {"use_tr16", "use_side_stream", "knob_convout_bands"} <= set(passed) and len(passed) >= 14, sorted(passed)
    missing = {n: f for n, f in passed.items() if n not in table}
    assert not missing, missing


def test_header_documents_the_table():
    table, doc = dict(option_table()), documented_options()
    assert doc, "no `name [default]` token in front of vae_set_option"
    wrong = [(n, d) for n, d in doc if table.get(n) != d]
    assert not wrong, wrong                                   # an unknown name, or another default than the table's
    names = [n for n, _ in doc]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)   # each option appears once
    assert not set(table) - set(names), sorted(set(table) - set(names))                   # and every table entry is documented
    assert table["knob_conv1_grid"] == 512 and table["use_fused_wgrad"] == 1


def test_set_option_refuses_a_null_context():
    L = _lib.lib()
    assert L.vae_set_option(None, b"use_tr16", 1) == -1 and b"null ctx" in L.vae_last_error()
