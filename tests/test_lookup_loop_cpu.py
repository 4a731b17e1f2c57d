"""Lookup decoding as one device loop, as far as a box without a GPU can check it: the two entry points are declared, exported and bound."""
import ctypes as C
import os

from support import E_ARG, ROOT, rwkv_mod  # noqa: F401


def test_entry_points_are_declared_exported_and_bound(built, rwkv_mod):
    from rwkv_cpp_accelerated_amd import engine
    lib = engine.lib()
    hdr = open(os.path.join(ROOT, "include", "rwkv_mi355x.h")).read()
    for name, n_args in (("rwkv_decode_lookup_streams", 8), ("rwkv_debug_lookup_draft", 8)):
        assert name + "(" in hdr and name in engine.ABI_SYMBOLS and len(getattr(lib, name).argtypes) == n_args
    assert "#define RWKV_MI355X_ABI_VERSION 6" in hdr and lib.rwkv_abi_version() == 6       # additions alone do not bump it
    assert "#define RWKV_LOOKUP_MAX_NGRAM 8u" in hdr and engine.LOOKUP_MAX_NGRAM == 8
    assert "#define RWKV_LOOKUP_MAX_HISTORY (1u << 20)" in hdr and engine.LOOKUP_MAX_HISTORY == 1 << 20
    assert C.sizeof(engine.LookupParams) == 16
    assert lib.rwkv_decode_lookup_streams(None, None, None, 1, 1, None, None, None) == E_ARG
    assert lib.rwkv_debug_lookup_draft(None, None, None, 1, 1, 1, None, None) == E_ARG
    assert callable(engine.RWKV.decode_lookup_device) and callable(engine.RWKV.debug_lookup_draft) and callable(rwkv_mod.decodeLookupStreams)
    assert "decodeLookupStreams(" in open(os.path.join(ROOT, "include", "rwkv.h")).read()
