"""rwkv_sample_rows and rwkv_spec_sample_segments as far as a box without a GPU can check them: declared, exported, bound in all three
interfaces, and refused without a context."""
import ctypes as C
import os

from support import E_ARG, ROOT, rwkv_mod  # noqa: F401


def test_entry_points_are_declared_exported_and_bound(built, rwkv_mod):
    from rwkv_cpp_accelerated_amd import engine
    lib = engine.lib()
    hdr = open(os.path.join(ROOT, "include", "rwkv_mi355x.h")).read()
    dropin = open(os.path.join(ROOT, "include", "rwkv.h")).read()
    for name, n_args in (("rwkv_sample_rows", 4), ("rwkv_spec_sample_segments", 11)):
        assert name + "(" in hdr and name in engine.ABI_SYMBOLS and len(getattr(lib, name).argtypes) == n_args
    assert C.sizeof(engine.PickQuery) == 88 and C.sizeof(engine.Pick) == 48
    assert lib.rwkv_sample_rows(None, None, 1, None) == E_ARG
    assert lib.rwkv_spec_sample_segments(None, None, None, 1, None, None, None, 0, None, None, None) == E_ARG
    assert callable(engine.RWKV.sample_rows) and callable(engine.RWKV.spec_sample_segments)
    assert callable(rwkv_mod.sampleRows) and callable(rwkv_mod.specSampleSegments)
    assert "sampleRows(" in dropin and "specSampleSegments(" in dropin
