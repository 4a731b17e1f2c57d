"""The device scorer's surface, as far as a box without a GPU can check it: rwkv_score_rows / rwkv_score are declared, exported and bound,
the Python methods and the pybind function exist, and tests/cpp/score_app.cpp compiles and links against include/rwkv.h.  (rwkv_create
needs a device, so the status codes of an unloaded context are checked by tests/test_score_gpu.py; a NULL context is checked here.)"""
import ctypes as C
import os
import subprocess

import pytest

from support import E_ARG, ROOT, build_app, rwkv_mod  # noqa: F401


@pytest.fixture(scope="module")
def score_app(built, tmp_path_factory):
    return build_app("score_app", tmp_path_factory.mktemp("cpp"))


def test_score_app_compiles_and_links(score_app):
    assert os.path.exists(score_app)
    syms = subprocess.run(["nm", "-D", "--undefined-only", score_app], capture_output=True, text=True).stdout
    assert "rwkv_score_rows" in syms and "rwkv_score\n" in syms + "\n"


def test_score_entry_points_are_declared_exported_and_bound(built):
    from rwkv_cpp_accelerated_amd import engine
    hdr = open(os.path.join(ROOT, "include", "rwkv_mi355x.h")).read()
    lib = engine.lib()
    for s in ("rwkv_score_rows", "rwkv_score"):
        assert s + "(" in hdr and s in engine.ABI_SYMBOLS and hasattr(lib, s), s
        assert len(getattr(lib, s).argtypes) == 7
    assert "#define RWKV_MAX_SCORE 65536u" in hdr and engine.MAX_SCORE == 65536
    assert "#define RWKV_MI355X_ABI_VERSION 6" in hdr and lib.rwkv_abi_version() == 6       # additions alone do not bump it
    for f in ("score_rows", "score", "_score"):
        assert callable(getattr(engine.RWKV, f, None)), f


def test_a_null_context_is_a_bad_argument(built):
    from rwkv_cpp_accelerated_amd import engine
    lib = engine.lib()
    one, lp = (C.c_uint64 * 1)(1), (C.c_double * 1)()
    assert lib.rwkv_score_rows(None, one, one, 1, lp, None, None) == E_ARG
    assert lib.rwkv_score(None, one, one, 1, lp, None, None) == E_ARG


def test_pybind_module_has_score_tokens(rwkv_mod):
    rwkv = rwkv_mod
    assert callable(getattr(rwkv, "scoreTokens", None))
    for f in ("initRwkv", "loadModel", "modelForward", "initState", "getState", "initOutput", "getOutput", "typicalSample"):
        assert hasattr(rwkv, f), f                      # the reference's names stay
