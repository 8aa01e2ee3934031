"""CPU checks of the device-resident snapshot API (include/procgen_mi355x.h procgen_store_*,
procgen_fork_envs): the built library exports the symbols with the declared signatures, and a NULL
handle is an error, not a crash -- without touching a GPU (the handle check precedes any HIP call)."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "procgen_mi355x.h")

# name -> (return type, parameter types after the handle) as the header declares them
DECLARED = {
    "procgen_store_create": ("int", ["int"]),
    "procgen_store_free": ("int", ["int"]),
    "procgen_store_save": ("int", ["int", "const int32_t *", "const int32_t *", "int"]),
    "procgen_store_load": ("int", ["int", "const int32_t *", "const int32_t *", "int"]),
    "procgen_fork_envs": ("int", ["const int32_t *", "const int32_t *", "int"]),
    "procgen_store_slot_bytes": ("int64_t", []),
}
CTYPE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "const int32_t *": ctypes.c_void_p}


def header_signature(name):
    src = open(HEADER).read()
    m = re.search(r"LIBENV_API\s+(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, "%s is not declared in procgen_mi355x.h" % name
    params = [re.sub(r"\s*\w+$", "", p.strip()) for p in m.group(2).split(",")]
    return m.group(1), params


@pytest.mark.parametrize("name", sorted(DECLARED))
def test_symbol_exported_with_declared_signature(name):
    from procgen_amd import _lib
    lib = _lib.load()
    res, params = header_signature(name)
    assert params[0] == "libenv_env *"
    assert (res, params[1:]) == DECLARED[name]
    fn = getattr(lib, name)  # AttributeError: the library does not export it
    want_res, want_args = _lib.SIGNATURES[name]
    assert want_res is CTYPE[res]
    assert want_args == [ctypes.c_void_p] + [CTYPE[p] for p in params[1:]]
    assert fn.restype is want_res and list(fn.argtypes) == want_args


def test_null_handle_is_an_error():
    from procgen_amd import _lib
    lib = _lib.load()
    ids = np.zeros(2, np.int32)
    p = ids.ctypes.data
    assert lib.procgen_store_create(None, 4) < 0
    assert lib.procgen_store_free(None, 0) < 0
    assert lib.procgen_store_save(None, 0, p, p, 2) < 0
    assert lib.procgen_store_load(None, 0, p, p, 2) < 0
    assert lib.procgen_fork_envs(None, p, p, 2) < 0
    assert lib.procgen_store_slot_bytes(None) < 0


def test_store_class_exported():
    import procgen_amd
    assert "SnapshotStore" in procgen_amd.__all__
    for m in ("save", "load", "save_all", "load_all", "close"):
        assert callable(getattr(procgen_amd.SnapshotStore, m))
    assert callable(procgen_amd.BaseProcgenEnv.snapshot_store) and callable(procgen_amd.BaseProcgenEnv.fork)
