"""Speculative greedy decoding, as far as a box without a GPU can check it: rwkv_spec_verify / rwkv_decode_speculative are declared, exported and
bound (ctypes, pybind, C++), tests/cpp/spec_app.cpp compiles and links, and the pure-Python statement of accept / commit and of the round loop
(tests/spec_cases.py) is run on the CPU oracle: whatever drafts, the output is the greedy continuation, and never more than n_tokens ids.  The
margin condition of the GPU suite's comparison with rwkv_decode_greedy is proved here on the oracle alone.  (rwkv_create needs a device, so the
status codes of a context are checked by the GPU suite; a NULL context is checked here.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import spec_cases as sc

from support import E_ARG, ROOT, build_app, headers_compile, rwkv_mod  # noqa: F401


@pytest.fixture(scope="module")
def om(oracle):
    """the oracle on the model of the comparison with plain decode, and the state behind its prompt"""
    from rwkv_cpp_accelerated_amd import modelfile as mf
    p = sc.PLAIN
    m = oracle.from_tensors(p["L"], p["D"], mf.synthetic_tensors(p["L"], p["D"], seed=p["seed"]))
    st = m.new_state()
    m.forward(list(p["prompt"]), st)
    ids, g = sc.gaps(m.forward, [s.copy() for s in st], p["first"], p["n"] + 1)
    yield m, st, ids, g
    m.close()


def test_entry_points_are_declared_exported_and_bound(built):
    from rwkv_cpp_accelerated_amd import engine
    hdr = open(os.path.join(ROOT, "include", "rwkv_mi355x.h")).read()
    lib = engine.lib()
    for s, nargs in (("rwkv_spec_verify", 6), ("rwkv_decode_speculative", 7)):
        assert s + "(" in hdr and s in engine.ABI_SYMBOLS and hasattr(lib, s), s
        assert len(getattr(lib, s).argtypes) == nargs
    syms = subprocess.run(["nm", "-D", "--defined-only", built["engine"]], capture_output=True, text=True).stdout
    assert " T rwkv_spec_verify" in syms and " T rwkv_decode_speculative" in syms
    assert "#define RWKV_SPEC_MAX_DRAFT 31u" in hdr and engine.SPEC_MAX_DRAFT == 31 == sc.MAX_DRAFT
    assert "#define RWKV_MI355X_ABI_VERSION 6" in hdr and lib.rwkv_abi_version() == 6       # additions alone do not bump it
    assert C.sizeof(engine.SpecStats) == 24
    for f in ("spec_verify", "decode_speculative", "decode_lookup"):
        assert callable(getattr(engine.RWKV, f, None)), f
    cpp = open(os.path.join(ROOT, "include", "rwkv.h")).read()
    assert "specVerify(" in cpp and "decodeSpeculative(" in cpp


def test_ctypes_signatures_match_the_header(built):
    """the argument lists of the two declarations, word for word, against the ctypes argtypes"""
    from rwkv_cpp_accelerated_amd import engine
    import re
    hdr = " ".join(open(os.path.join(ROOT, "include", "rwkv_mi355x.h")).read().split())
    lib = engine.lib()
    u64, vp = C.c_uint64, C.c_void_p
    kinds = {"rwkv_ctx *": vp, "uint64_t": u64, "uint32_t": C.c_uint32, "const uint64_t *": C.POINTER(u64), "uint64_t *": C.POINTER(u64),
             "rwkv_spec_stats *": C.POINTER(engine.SpecStats)}
    for name in ("rwkv_spec_verify", "rwkv_decode_speculative"):
        m = re.search(r"int " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        args = [re.sub(r"/\*.*?\*/", "", a).strip() for a in m.group(1).split(",")]
        want = [kinds[re.sub(r"\s*\w+$", "", a).strip() if not a.endswith("*") else a] for a in args]
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == want, (name, args)


def test_a_null_context_is_a_bad_argument(built):
    from rwkv_cpp_accelerated_amd import engine
    lib = engine.lib()
    out, d = (C.c_uint64 * 4)(), (C.c_uint64 * 2)(5, 6)
    assert lib.rwkv_spec_verify(None, 5, d, 2, out, out) == E_ARG
    assert lib.rwkv_decode_speculative(None, None, 5, 4, 2, out, None) == E_ARG


def test_headers_compile(built, tmp_path):
    headers_compile(tmp_path)


def test_pybind_module_has_the_spec_functions(rwkv_mod):
    rwkv = rwkv_mod
    for f in ("specVerify", "decodeSpeculative"):
        assert callable(getattr(rwkv, f, None)), f


def test_spec_app_compiles_and_links(built, tmp_path):
    app = build_app("spec_app", tmp_path)
    syms = subprocess.run(["nm", "-D", "--undefined-only", app], capture_output=True, text=True).stdout
    assert "rwkv_spec_verify" in syms and "rwkv_decode_speculative" in syms


def test_pick_rule():
    r = np.full(sc.V, -1.0, np.float32)
    r[0] = 9.0; r[7] = r[9] = 3.0
    assert sc.pick(r) == 7                                       # logit 0 banned, ties to the lowest id
    r[:] = -np.inf; r[0] = 1.0
    assert sc.pick(r) == 0                                       # no winner
    r[:] = np.nan
    assert sc.pick(r) == 0
    r[:] = -np.inf; r[sc.V - 1] = -3e38
    assert sc.pick(r) == sc.V - 1


def test_accept():
    assert sc.accept([], [4]) == 0
    assert sc.accept([4, 5, 6], [4, 5, 6, 7]) == 3
    assert sc.accept([4, 9, 6], [4, 5, 6, 7]) == 1
    assert sc.accept([0, 5], [4, 5, 6]) == 0


def test_margin_condition_on_the_oracle_alone(om):
    _, _, ids, g = om
    print(f"continuation {ids[:8]} ..; smallest top-two gap / max |logit| over {len(g)} steps: {min(g):.3e}")
    assert min(g) >= sc.MARGIN
    assert all(0 < t < sc.V for t in ids)


def test_verify_statement_rolls_back_exactly(om):
    m, st0, g, _ = om
    first = sc.PLAIN["first"]
    for n_draft in (1, 2, 7):
        for label, d, a_want in sc.planted(g, n_draft):
            st = [s.copy() for s in st0]
            a, nx, picks = sc.verify(m.forward, st, first, d)
            assert (a, nx) == (a_want, g[a_want]), (n_draft, label)
            want = [s.copy() for s in st0]
            m.forward([first] + g[:a_want], want)
            assert all(np.array_equal(x, y) for x, y in zip(st, want)), (n_draft, label)


@pytest.mark.parametrize("k", [1, 4, 31])
def test_loop_gives_the_greedy_continuation_for_any_draft(om, k):
    from rwkv_cpp_accelerated_amd import engine
    m, st0, g, _ = om
    first, n = sc.PLAIN["first"], 24
    rng = np.random.default_rng(k)
    sources = dict(
        perfect=lambda h, kd: g[len(h) - 1:len(h) - 1 + kd],
        wrong=lambda h, kd: [int(t) for t in rng.integers(1, sc.V, kd)],
        half=lambda h, kd: (g[len(h) - 1:len(h) - 1 + kd // 2] + [1] * kd)[:kd],
        zeros=lambda h, kd: [0] * kd,
        lookup=lambda h, kd: engine.ngram_draft(h, kd, 2),
        short=lambda h, kd: g[len(h) - 1:len(h)],
    )
    for name, src in sources.items():
        for n_tokens in (1, k, n):
            st = [s.copy() for s in st0]
            ids, stats = sc.loop(lambda t, d: sc.verify(m.forward, st, t, d), src, first, n_tokens, k)
            assert ids == g[:n_tokens], (name, n_tokens)
            assert stats["accepted"] <= stats["drafted"] and stats["rounds"] <= n_tokens
            want = [s.copy() for s in st0]
            m.forward([first] + g[:n_tokens - 1], want)           # consumed: first, ids[:-1] -- never more
            assert all(np.array_equal(x, y) for x, y in zip(st, want)), (name, n_tokens)
        if name == "perfect":
            assert stats["accepted"] == stats["drafted"] and stats["rounds"] == -(-n // (k + 1))
        if name in ("wrong", "zeros"):
            assert stats["accepted"] == 0 and stats["rounds"] == n


def test_ngram_draft_on_hand_made_histories():
    from rwkv_cpp_accelerated_amd.engine import ngram_draft
    assert ngram_draft([1, 2, 3, 4, 5], 4, 3) == []                              # no match
    assert ngram_draft([1, 2, 3], 4, 3) == [] and ngram_draft([], 4, 3) == []    # too short to have an earlier occurrence
    assert ngram_draft([1, 2, 3, 9, 8, 1, 2, 3], 4, 3) == [9, 8, 1, 2]           # what followed the earlier occurrence
    assert ngram_draft([1, 2, 3, 9, 8, 1, 2, 3], 2, 3) == [9, 8]                 # at most k
    assert ngram_draft([7, 1, 2, 3, 1, 2, 3], 4, 3) == [1, 2, 3]                 # a match at the very end: what follows runs into the tail
    assert ngram_draft([5, 5, 5, 5], 4, 3) == [5]                                # overlapping matches: the most recent one, one id behind it
    assert ngram_draft([5, 5, 5, 5, 5], 4, 2) == [5]
    assert ngram_draft([1, 2, 7, 1, 2, 8, 1, 2], 1, 2) == [8]                    # the MOST RECENT earlier occurrence
    assert ngram_draft([1, 2, 7, 1, 2], 3, 2) == [7, 1, 2]
    assert ngram_draft([1, 2, 7, 1, 2], 0, 2) == [] and ngram_draft([1, 2, 7, 1, 2], 3, 0) == []
