"""Log-probs and top-n alternatives, as far as a box without a GPU can check them: rwkv_topn_rows / rwkv_decode_batch_logprobs are declared,
exported and bound, the Python methods and the pybind function exist, tests/cpp/logprobs_app.cpp compiles and links against include/rwkv.h,
and the numpy reference of tests/logprob_cases.py -- what tests/test_logprobs_gpu.py holds the kernels to -- is itself held to half the
bound against an np.longdouble evaluation, with its tie order pinned.  (rwkv_create needs a device, so the status codes of a context are
checked by the GPU suite; a NULL context is checked here.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import logprob_cases as lc
import score_cases as sc

from support import E_ARG, ROOT, build_app, rwkv_mod  # noqa: F401


def test_entry_points_are_declared_exported_and_bound(built):
    from rwkv_cpp_accelerated_amd import engine
    hdr = open(os.path.join(ROOT, "include", "rwkv_mi355x.h")).read()
    lib = engine.lib()
    for s, nargs in (("rwkv_topn_rows", 6), ("rwkv_decode_batch_logprobs", 12)):
        assert s + "(" in hdr and s in engine.ABI_SYMBOLS and hasattr(lib, s), s
        assert len(getattr(lib, s).argtypes) == nargs
    assert "#define RWKV_MAX_TOPN 32u" in hdr and engine.TOPN_MAX == 32 == lc.TOPN_MAX
    assert "#define RWKV_MAX_LOGPROB_ENTRIES (1u << 22)" in hdr and engine.LOGPROB_ENTRIES_MAX == 1 << 22
    assert 96 * 2048 * (1 + 20) <= engine.LOGPROB_ENTRIES_MAX                                # the header's example fits
    assert "#define RWKV_MI355X_ABI_VERSION 6" in hdr and lib.rwkv_abi_version() == 6       # additions alone do not bump it
    assert C.sizeof(engine.LogprobOut) == 40
    for f in ("topn_rows", "decode_batch_logprobs"):
        assert callable(getattr(engine.RWKV, f, None)), f


def test_a_null_context_is_a_bad_argument(built):
    from rwkv_cpp_accelerated_amd import engine
    lib = engine.lib()
    one, lp, ids, ln = (C.c_uint64 * 1)(1), (C.c_double * 1)(), (C.c_uint64 * 1)(), (C.c_uint32 * 1)()
    assert lib.rwkv_topn_rows(None, one, 1, 1, ids, lp) == E_ARG
    pk = engine.Pick(engine.PICK_GREEDY, 1.0, 0.8, 0, engine.nucleus_params())
    rec = engine.LogprobOut(0, 0, lp, None, None, None)
    assert lib.rwkv_decode_batch_logprobs(None, one, 1, 1, C.byref(pk), None, None, C.byref(rec), ids, ln, None, None) == E_ARG


def test_pybind_module_has_top_logprobs(rwkv_mod):
    rwkv = rwkv_mod
    assert callable(getattr(rwkv, "topLogprobs", None))
    for f in ("initRwkv", "loadModel", "modelForward", "initState", "getState", "initOutput", "getOutput", "typicalSample", "scoreTokens"):
        assert hasattr(rwkv, f), f                      # the reference's names stay


def test_logprobs_app_compiles_and_links(built, tmp_path):
    app = build_app("logprobs_app", tmp_path)
    syms = subprocess.run(["nm", "-D", "--undefined-only", app], capture_output=True, text=True).stdout
    assert "rwkv_decode_batch_logprobs" in syms and "rwkv_topn_rows" in syms


@pytest.mark.parametrize("name", lc.CASES)
def test_reference_against_longdouble_at_half_the_bound(name):
    ids, lp = lc.ref_of(name)
    ids_l, lp_l = lc.topn_reference(lc.logits_of(name), lc.TOPN_MAX, np.longdouble)
    assert np.array_equal(ids, ids_l)
    l = lc.logits_of(name)
    assert np.all(l[ids][1:] <= l[ids][:-1]) and len(set(ids.tolist())) == lc.TOPN_MAX
    assert l[ids[-1]] >= np.delete(l, ids).max()                   # nothing left out beats the last one kept
    inf = np.isneginf(lp_l)
    assert np.array_equal(np.isneginf(lp), inf)
    d = np.abs((lp[~inf].astype(np.longdouble) - lp_l[~inf]).astype(np.float64))
    print(f"{name:>14}: worst |f64 - longdouble| {d.max() if d.size else 0.0:.2e}   -inf entries {int(inf.sum())}")
    assert np.all(d <= sc.LP_TOL / 2)


def test_tie_order_is_pinned():
    V = lc.V
    assert lc.topn_reference(lc.logits_of("ties"), 5)[0].tolist() == [0, 1, 49, 50, 51]
    assert lc.ref_of("ties")[0].tolist() == [0, 1, 49, 50, 51, V - 1] + list(range(2, 28))
    for n in lc.TOP_NS:
        assert lc.topn_reference(lc.logits_of("const"), n)[0].tolist() == list(range(n))
    assert lc.ref_of("straddle")[0][:6].tolist() == [3140, 3141, 3142, 3143, 47133, 47134]
    assert lc.ref_of("tail")[0].tolist() == list(range(V - 1, V - 33, -1))
    assert lc.ref_of("one_per_slice")[0][:16].tolist() == [lc.slice_lo(b) + 100 + 7 * b for b in range(15, -1, -1)]
    ids, lp = lc.ref_of("few_finite")
    assert ids.tolist() == [3142, 7, V - 1] + list(range(0, 7)) + list(range(8, 30)) and np.isneginf(lp[3:]).all() and np.isfinite(lp[:3]).all()
