"""Draft trees for many streams, as far as a box without a GPU can check them: rwkv_tree_plan, the one validator, on the table of refused calls; engine.ngram_draft_tree on three hand-written histories; and the margin condition of the GPU suite's oracle case,
proved here on the oracle alone."""
import ctypes as C

import numpy as np
import pytest

import segment_cases as sg
import spec_cases as sc
import specseg_cases as cs
import spectree_cases as tc
from support import E_ARG


@pytest.mark.parametrize("segs,ids,parent,pick,text", [r for r in tc.REFUSED if r[3] is None])
def test_tree_plan_refuses(built, segs, ids, parent, pick, text):
    from rwkv_cpp_accelerated_amd import engine
    lib = engine.lib()
    out = np.full(64, 77, np.uint8)
    u8 = out.ctypes.data_as(C.POINTER(C.c_uint8))
    assert lib.rwkv_tree_plan(*tc.refused_args(engine, segs, ids, parent), cs.MAXT, 64, u8, u8, None) == E_ARG
    assert text in lib.rwkv_last_error().decode() and (out == 77).all(), lib.rwkv_last_error()


@pytest.mark.parametrize("history,k,branches,want", [
    # branching: the tail 1 2 occurred three times (7 9 1 2, 3 5 9 1 .., 3 4 9 1 ..): level by level, the newest first, equal prefixes merged
    ([1, 2, 3, 4, 9, 1, 2, 3, 5, 9, 1, 2, 7, 9, 1, 2], 8, 3, ([7, 3, 9, 5, 4, 1, 9, 9], [-1, -1, 0, 1, 1, 2, 3, 4])),
    ([1, 2, 3, 4, 9, 1, 2, 3, 5, 9, 1, 2, 7, 9, 1, 2], 8, 2, ([7, 3, 9, 5, 1, 9, 2, 1], [-1, -1, 0, 1, 2, 3, 4, 5])),
    ([4, 1, 2, 8, 6, 1, 2], 3, 3, ([8, 6, 1], [-1, 0, 1])),      # one occurrence: ngram_draft's chain
    ([1, 2, 3, 4, 5], 4, 3, ([], [])),                              # no occurrence
])
def test_ngram_draft_tree(history, k, branches, want):
    from rwkv_cpp_accelerated_amd import engine
    ids, parent = engine.ngram_draft_tree(history, k, 2, branches)
    assert (ids, parent) == want


def test_margin_condition_on_the_oracle_alone(oracle):
    """the planted trees of the GPU suite's oracle case from the oracle's own start state: every row on a path has a top-two gap of at least MARGIN"""
    from rwkv_cpp_accelerated_amd import modelfile as mf
    L, D = cs.WIDTHS[0]
    om = oracle.from_tensors(L, D, mf.synthetic_tensors(L, D, seed=cs.SEED + D))
    calls = []                                                     # segment_cases.start_state itself, recorded: a PARRALEL history, a GPT prompt on slot 0
    rec = type("Recorded", (), dict(MODE_PARRALEL="par", MODE_GPT="gpt", forward=staticmethod(lambda ids, mode: calls.append((list(ids), mode)))))
    sg.start_state(rec, rec, D)
    (history, _), (prompt, _) = calls
    for slot, nc in tc.HEADS[32]:
        st = om.new_state()
        om.forward([history[slot]] + (prompt if slot == 0 else []), st)
        l = om.forward(cs.certain(slot, nc), st)[-1]
        for d in range(tc.DEPTH):
            assert cs.gap(l) >= cs.MARGIN, (slot, d, cs.gap(l))
            l = om.forward([sc.pick(l)], st)[0]
    om.close()
