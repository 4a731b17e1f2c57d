"""Lookup decoding with draft trees as one device loop, as far as a box without a GPU can check it: the two entry points are declared, exported
and bound."""
import ctypes as C
import os

from support import E_ARG, ROOT, rwkv_mod  # noqa: F401


def test_entry_points_are_declared_exported_and_bound(built, rwkv_mod):
    from rwkv_cpp_accelerated_amd import engine
    lib = engine.lib()
    hdr = open(os.path.join(ROOT, "include", "rwkv_mi355x.h")).read()
    for name, n_args in (("rwkv_decode_lookup_trees", 8), ("rwkv_debug_lookup_tree", 10)):
        assert name + "(" in hdr and name in engine.ABI_SYMBOLS and len(getattr(lib, name).argtypes) == n_args
    assert "#define RWKV_MI355X_ABI_VERSION 6" in hdr and lib.rwkv_abi_version() == 6       # additions alone do not bump it
    assert "#define RWKV_LOOKUP_MAX_BRANCHES 8u" in hdr and engine.LOOKUP_MAX_BRANCHES == 8
    assert C.sizeof(engine.LookupTreeParams) == 16 and [f[0] for f in engine.LookupTreeParams._fields_] == ["k", "n", "branches", "flags"]
    assert lib.rwkv_decode_lookup_trees(None, None, None, 1, 1, None, None, None) == E_ARG
    assert lib.rwkv_debug_lookup_tree(None, None, None, 1, 1, 1, 1, None, None, None) == E_ARG
    assert callable(engine.RWKV.decode_lookup_tree_device) and callable(engine.RWKV.debug_lookup_tree) and callable(rwkv_mod.decodeLookupTrees)
    assert "decodeLookupTrees(" in open(os.path.join(ROOT, "include", "rwkv.h")).read()
