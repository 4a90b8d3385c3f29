"""Interfaces of the differentiable encode / decode / eval-mode paths (no GPU needed): the C header declares the new entry
points with the argument types tests/test_grad_paths_gpu.py drives them through, and _lib binds them the same way."""
import ctypes as C
import os
import re

from torch_vae_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vae_step.h")

# C parameter type -> ctypes argument type of _lib
CTYPES = {"vae_ctx*": C.c_void_p, "const float*": C.c_void_p, "float*": C.c_void_p, "float": C.c_float, "int": C.c_int,
          "int64_t*": C.c_void_p, "uint64_t": C.c_uint64, "vae_stream_t": C.c_void_p}


def declared_params(name):
    text = open(HEADER).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/vae_step.h"
    params = []
    for p in m.group(1).split(","):
        p = " ".join(p.split())
        typ = re.sub(r"\s*\b\w+$", "", p).replace(" *", "*")
        params.append(typ)
    return params


def test_header_declares_new_entry_points():
    enc = declared_params("vae_encode")
    assert enc == ["vae_ctx*", "const float*", "int", "const float*", "float*", "int64_t*", "const float*", "uint64_t", "int",
                   "float*", "float*", "float*", "vae_stream_t"]
    bwd = declared_params("vae_backward_ex")
    # vae_backward's arguments, then dx and dz, then the stream
    assert bwd[:-3] == declared_params("vae_backward")[:-1]
    assert bwd[-3:] == ["float*", "float*", "vae_stream_t"]


def test_lib_binds_them_with_matching_types():
    assert "vae_encode" in _lib.EXPORTS and "vae_backward_ex" in _lib.EXPORTS
    src = open(_lib.__file__).read()
    for name in ("vae_encode", "vae_backward_ex"):
        m = re.search(r"_sig\(L\." + name + r", i32, \[([^\]]*)\]\)", src)
        assert m, name
        names = [a.strip() for a in m.group(1).split(",")]
        alias = {"p": C.c_void_p, "i32": C.c_int, "u64": C.c_uint64, "f32": C.c_float}
        assert [alias[a] for a in names] == [CTYPES[t] for t in declared_params(name)], name
