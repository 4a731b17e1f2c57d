"""Segmented forward, as far as a box without a GPU can check it: rwkv_forward_segments / rwkv_segment_plan are declared, exported and bound
(ctypes, pybind, C++), tests/cpp/segments_app.cpp compiles and links, the host-only validator equals its Python statement on every layout of
tests/segment_cases.py and rejects what the header says it rejects, and the statement of the call is run on the CPU oracle: one segment is GPT
mode, segments of length 1 are PARRALEL mode, and a mix equals its segments run alone.  (rwkv_create needs a device, so the status codes of a
context are checked by the GPU suite; a NULL context is checked here.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib
import segment_cases as sg

from support import E_ARG, ROOT, build_app, headers_compile, rwkv_mod  # noqa: F401


def test_entry_points_are_declared_exported_and_bound(built):
    from rwkv_cpp_accelerated_amd import engine
    hdr = open(os.path.join(ROOT, "include", "rwkv_mi355x.h")).read()
    lib = engine.lib()
    for s, nargs in (("rwkv_forward_segments", 6), ("rwkv_segment_plan", 6)):
        assert s + "(" in hdr and s in engine.ABI_SYMBOLS and hasattr(lib, s), s
        assert len(getattr(lib, s).argtypes) == nargs
    syms = subprocess.run(["nm", "-D", "--defined-only", built["engine"]], capture_output=True, text=True).stdout
    assert " T rwkv_forward_segments" in syms and " T rwkv_segment_plan" in syms
    assert "#define RWKV_MI355X_ABI_VERSION 6" in hdr and lib.rwkv_abi_version() == 6       # additions alone do not bump it
    assert "typedef struct rwkv_segment { uint32_t slot; uint32_t n; } rwkv_segment;" in hdr and C.sizeof(engine.Segment) == 8
    for f in ("forward_segments",):
        assert callable(getattr(engine.RWKV, f, None)), f
    assert callable(engine.segment_plan)
    cpp = open(os.path.join(ROOT, "include", "rwkv.h")).read()
    assert "forwardSegments(" in cpp and "struct Segment {" in cpp


def test_a_null_context_is_a_bad_argument(built):
    from rwkv_cpp_accelerated_amd import engine
    lib = engine.lib()
    toks, segs, last = (C.c_uint64 * 2)(5, 6), (engine.Segment * 1)(engine.Segment(0, 2)), (C.c_uint64 * 1)()
    assert lib.rwkv_forward_segments(None, toks, segs, 1, 0, last) == E_ARG


def test_headers_compile(built, tmp_path):
    headers_compile(tmp_path)


def test_pybind_module_has_the_function(rwkv_mod):
    rwkv = rwkv_mod
    assert callable(getattr(rwkv, "modelForwardSegments", None))


def test_segments_app_compiles_and_links(built, tmp_path):
    app = build_app("segments_app", tmp_path)
    syms = subprocess.run(["nm", "-D", "--undefined-only", app], capture_output=True, text=True).stdout
    assert "rwkv_forward_segments" in syms and "rwkv_score_rows" in syms


def _plan(lib, engine, layout, max_ctx, n_segs=None, null_segs=False):
    """(status, row_slot, row_flags, n_rows) of the C call; the outputs start as 0xEE.. patterns so that a write shows"""
    segs = (engine.Segment * max(1, len(layout)))(*[engine.Segment(s, n) for s, n in layout])
    cap = max(1, sum(n for _, n in layout)) + 8
    slot, flags, T = np.full(cap, 0xEEEEEEEE, np.uint32), np.full(cap, 0xEE, np.uint8), C.c_uint64(0xEEEE)
    rc = lib.rwkv_segment_plan(None if null_segs else segs, len(layout) if n_segs is None else n_segs, max_ctx,
                               slot.ctypes.data_as(C.POINTER(C.c_uint32)), flags.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(T))
    return rc, slot, flags, int(T.value)


@pytest.mark.parametrize("name", list(sg.LAYOUTS))
def test_plan_equals_its_statement(built, name):
    from rwkv_cpp_accelerated_amd import engine
    layout = sg.LAYOUTS[name]
    want_slot, want_flags = sg.segment_plan(layout, sg.MAXT)
    T = sg.ROWS[name]
    assert len(want_slot) == T == sum(n for _, n in layout)
    rc, slot, flags, n_rows = _plan(engine.lib(), engine, layout, sg.MAXT)
    assert rc == 0 and n_rows == T
    assert np.array_equal(slot[:T], want_slot) and np.array_equal(flags[:T], want_flags)
    assert (slot[T:] == 0xEEEEEEEE).all() and (flags[T:] == 0xEE).all()          # nothing behind row T - 1
    s2, f2 = engine.segment_plan(layout, sg.MAXT)                                 # the binding, and validate-only inside it
    assert np.array_equal(s2, want_slot) and np.array_equal(f2, want_flags)
    # what the flags say: row 0 of every pass is a first row and its last row a last row; every segment starts first and ends last
    assert all(want_flags[j] & sg.FIRST for j in range(0, T, sg.PASS_ROWS)) and want_flags[T - 1] & sg.LAST
    assert all(want_flags[j] & sg.LAST for j in range(sg.PASS_ROWS - 1, T, sg.PASS_ROWS))


def test_plan_of_hand_made_lists(built):
    F, L_ = sg.FIRST, sg.LAST
    assert sg.segment_plan([(4, 3), (1, 1)], 8)[1].tolist() == [F, 0, L_, F | L_]
    s, f = sg.segment_plan([(2, 10)], 80, pass_rows=4)                           # pieces of 4, 4, 2
    assert f.tolist() == [F, 0, 0, L_, F, 0, 0, L_, F, L_] and set(s.tolist()) == {2}
    s, f = sg.segment_plan(sg.LAYOUTS["MIX77"], sg.MAXT)
    assert f[63] == L_ and f[64] == F and s[63] == s[64] == 2                    # (2, 10) is cut at the pass boundary: rows 60 .. 63 | 64 .. 69
    assert f[31] == 0 == f[32]                                                   # a half boundary cuts nothing
    s, f = sg.segment_plan(sg.LAYOUTS["MIX64"], sg.MAXT)
    assert s[30:34].tolist() == [1, 1, 1, 1] and f[30:34].tolist() == [F, 0, 0, L_]


def test_plan_rejects_and_writes_nothing(built):
    from rwkv_cpp_accelerated_amd import engine
    lib = engine.lib()
    bad = dict(
        duplicate_slot=dict(layout=[(3, 2), (5, 1), (3, 1)]),
        empty_segment=dict(layout=[(3, 2), (5, 0)]),
        slot_is_max_ctx=dict(layout=[(sg.MAXT, 1)]),
        too_many_rows=dict(layout=[(0, 40), (1, 41)]),
        no_segments=dict(layout=[(0, 1)], n_segs=0),
        null_segs=dict(layout=[(0, 1)], null_segs=True),
    )
    for name, kw in bad.items():
        rc, slot, flags, n_rows = _plan(lib, engine, kw["layout"], sg.MAXT, kw.get("n_segs"), kw.get("null_segs", False))
        err = lib.rwkv_last_error().decode()
        print(f"{name}: status {rc}, {err!r}")
        assert rc == E_ARG, name
        assert (slot == 0xEEEEEEEE).all() and (flags == 0xEE).all() and n_rows == 0xEEEE, name
        if "n_segs" not in kw and not kw.get("null_segs"):
            assert sg.segment_plan(kw["layout"], sg.MAXT) is None, name
            with pytest.raises(engine.RWKVError):
                engine.segment_plan(kw["layout"], sg.MAXT)
    assert sg.segment_plan([], sg.MAXT) is None
    rc, _, _, n_rows = _plan(lib, engine, [(0, 40), (1, 40)], sg.MAXT)            # T == max_ctx is allowed
    assert rc == 0 and n_rows == sg.MAXT
    segs = (engine.Segment * 1)(engine.Segment(7, 3))                             # validate only: every output NULL
    assert lib.rwkv_segment_plan(segs, 1, sg.MAXT, None, None, None) == 0


# ---- the statement over the CPU oracle ----
@pytest.fixture(scope="module")
def om(oracle):
    """the oracle on the narrowest model of the width cases, and a state with history on all 80 slots"""
    from rwkv_cpp_accelerated_amd import modelfile as mf
    L, D = sg.WIDTHS[0]
    m = oracle.from_tensors(L, D, mf.synthetic_tensors(L, D, seed=sg.SEED + D))
    st = m.new_state(sg.MAXT)
    rng = np.random.default_rng(D)
    m.forward([int(v) for v in rng.integers(1, sg.V, sg.MAXT)], st, mode=oracle_lib.MODE_PARRALEL)      # PARRALEL: a history on every slot
    m.forward([7, 50000, 11, 9], st)                                             # and a prompt on slot 0
    yield m, [s.reshape(sg.MAXT, L * D) for s in st]
    m.close()


def _copy(state):
    return [s.copy() for s in state]


def test_one_segment_is_gpt_mode(om):
    m, st0 = om
    for name in ("S2", "S33"):
        segs = sg.tokens_for(sg.LAYOUTS[name], 1)
        a, b = _copy(st0), _copy(st0)
        got = sg.forward_segments(m.forward, a, segs)
        flat = [s.reshape(-1) for s in b]                                        # (views: the oracle advances b in place)
        want = m.forward(segs[0][1], flat)
        assert np.array_equal(got, want), name
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), name


def test_segments_of_one_row_are_parralel_mode(om):
    m, st0 = om
    segs = sg.tokens_for(sg.LAYOUTS["PAR40"], 2)
    a, b = _copy(st0), _copy(st0)
    got = sg.forward_segments(m.forward, a, segs)
    want = m.forward([ids[0] for _, ids in segs], [s.reshape(-1) for s in b], mode=oracle_lib.MODE_PARRALEL)
    assert np.array_equal(got, want)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_a_mix_equals_its_segments_alone(om):
    m, st0 = om
    segs = sg.tokens_for(sg.LAYOUTS["MIX32"], 3)
    a = _copy(st0)
    got = sg.forward_segments(m.forward, a, segs)
    assert sg.last_rows(segs) == [0, 7, 8, 31]
    row = 0
    for slot, ids in segs:
        b = _copy(st0)
        alone = sg.forward_segments(m.forward, b, [(slot, ids)])
        assert np.array_equal(got[row:row + len(ids)], alone), slot
        assert all(np.array_equal(x[slot], y[slot]) for x, y in zip(a, b)), slot
        others = [s for s in range(sg.MAXT) if s != slot]
        assert all(np.array_equal(y[others], z[others]) for y, z in zip(b, st0)), slot
        row += len(ids)
