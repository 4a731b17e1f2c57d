"""Beam search, as far as a box without a GPU can check it: rwkv_decode_beam / rwkv_state_permute / rwkv_debug_beam_step are declared, exported and
bound (ctypes, pybind, C++), tests/cpp/beam_app.cpp compiles and links, and the HOST TWIN of the selection (include/rwkv_sampler.h beam_select, reached
through the pybind module's beamSelect) is held to the brute-force np.longdouble reference of tests/beam_cases.py -- which sorts all W x 50276
candidates, so that pruning to the rows' top W + 1 is shown to lose nothing -- with the tie order pinned and the margin condition asserted on the
reference alone.  (rwkv_create needs a device, so the status codes of a context are checked by the GPU suite; a NULL context is checked here.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import beam_cases as bc

from support import E_ARG, ROOT, build_app, rwkv_mod  # noqa: F401
V = bc.V


def twin(rwkv_mod, name, r):
    """the host twin on the case's rows, fed their top W + 1 from the numpy f64 reference"""
    rows, cum, ended, last, stops = bc.shifted(name, r)
    ids, lp = bc.rows_topn(rows, len(rows) + 1)
    return rwkv_mod.beamSelect(ids, lp, np.array(cum, np.float64), list(ended), list(last), list(stops))


def test_entry_points_are_declared_exported_and_bound(built):
    from rwkv_cpp_accelerated_amd import engine
    hdr = open(os.path.join(ROOT, "include", "rwkv_mi355x.h")).read()
    lib = engine.lib()
    for s, nargs in (("rwkv_decode_beam", 5), ("rwkv_state_permute", 3), ("rwkv_debug_beam_step", 10)):
        assert s + "(" in hdr and s in engine.ABI_SYMBOLS and hasattr(lib, s), s
        assert len(getattr(lib, s).argtypes) == nargs
    assert "#define RWKV_MAX_BEAM 16u" in hdr and engine.BEAM_MAX == 16
    assert "#define RWKV_BEAM_MAX_STOP 16u" in hdr and engine.BEAM_MAX_STOP == 16
    assert "#define RWKV_MI355X_ABI_VERSION 6" in hdr and lib.rwkv_abi_version() == 6       # additions alone do not bump it
    assert C.sizeof(engine.BeamParams) == 24 and C.sizeof(engine.BeamOut) == 32
    for f in ("decode_beam", "state_permute", "debug_beam_step"):
        assert callable(getattr(engine.RWKV, f, None)), f
    cpp = open(os.path.join(ROOT, "include", "rwkv.h")).read()
    assert "decodeBeam(" in cpp and "permuteState(" in cpp and "struct Beam " in cpp
    assert "beam_select(" in open(os.path.join(ROOT, "include", "rwkv_sampler.h")).read()
    for out in ("a length penalty", "stop sequences longer than one token", "sampling or penalties inside a beam", "ending the call early"):
        assert out in " ".join(hdr.split()), out                                             # the header says what is out of scope


def test_a_null_context_is_a_bad_argument(built):
    from rwkv_cpp_accelerated_amd import engine
    lib = engine.lib()
    tok, ln, sc_, par = (C.c_uint64 * 4)(), (C.c_uint32 * 2)(), (C.c_double * 2)(), (C.c_uint32 * 2)(0, 1)
    bp, alive = engine.beam_params(2)
    out = engine.BeamOut(tok, ln, sc_, None)
    assert lib.rwkv_decode_beam(None, 5, 2, C.byref(bp), C.byref(out)) == E_ARG
    assert lib.rwkv_state_permute(None, par, 2) == E_ARG
    cum, end, u8 = (C.c_double * 2)(), (C.c_uint8 * 2)(), (C.c_uint8 * 2)()
    assert lib.rwkv_debug_beam_step(None, C.byref(bp), cum, end, tok, par, tok, sc_, sc_, u8) == E_ARG
    del alive


def test_pybind_module_has_the_beam_functions(rwkv_mod):
    for f in ("decodeBeam", "beamSelect", "topLogprobs", "loadModel"):
        assert callable(getattr(rwkv_mod, f, None)), f


def test_beam_app_compiles_and_links(built, tmp_path):
    app = build_app("beam_app", tmp_path)
    syms = subprocess.run(["nm", "-D", "--undefined-only", app], capture_output=True, text=True).stdout
    assert "rwkv_decode_beam" in syms and "rwkv_state_permute" in syms


@pytest.mark.parametrize("name,r", bc.case_shifts())
def test_margin_condition_on_the_reference_alone(name, r):
    gaps = bc.margins(name, r)
    print(f"{name:>14} shift {r}: gaps {[float(g) for g in gaps]}")
    assert np.all((gaps == 0) | (gaps >= bc.MARGIN)), gaps


@pytest.mark.parametrize("name,r", bc.case_shifts())
def test_host_twin_against_the_brute_force_reference(rwkv_mod, name, r):
    want = bc.reference(name, r)
    got = twin(rwkv_mod, name, r)
    worst, bad = bc.check(f"{name} shift {r}", got, want)
    print(f"{name:>14} shift {r}: worst |d score| {worst:.2e}  parents {want['parent'].tolist()}  tokens {want['token'].tolist()}")
    assert not bad, bad
    assert np.all(np.diff(np.asarray(got[2])) <= 0)                                          # the beams are sorted


def test_tie_order_is_pinned(rwkv_mod):
    # bitwise-equal rows under equal cum: the best id of every row, by ascending parent
    w = bc.reference("equal_w5")
    assert w["parent"].tolist() == [0, 1, 2, 3, 4] and len(set(w["token"].tolist())) == 1
    assert len(set(float(s) for s in w["score"])) == 1
    assert np.asarray(twin(rwkv_mod, "equal_w5", 0)[0]).tolist() == [0, 1, 2, 3, 4]
    assert bc.reference("equal_w16")["parent"].tolist() == list(range(16))
    # equal logits inside a row: ascending id, id 0 dropped, and the cut falls between two of them
    w = bc.reference("id0_w5")
    assert w["parent"].tolist() == [0] * 5 and w["token"].tolist() == [1, 49, 50, 51, V - 1] and w["ended"].tolist() == [0, 0, 0, 0, 1]
    w = bc.reference("const_w5")
    assert w["parent"].tolist() == [0] * 5 and w["token"].tolist() == [1, 2, 3, 4, 5] and bc.margins("const_w5")[-1] == 0
    w = bc.reference("cut_w2")
    assert w["parent"].tolist() == [1, 0] and w["token"][1] == V - 2 and w["ended"].tolist() == [0, 1] and bc.margins("cut_w2")[-1] == 0
    # ended rows: one candidate each at their own score, equal scores by parent; an ended row stays ended
    w = bc.reference("ended_w5")
    assert w["parent"].tolist()[:2] == [1, 4] and w["token"].tolist()[:2] == [222, 555] and w["ended"].tolist()[:2] == [1, 1]
    assert [float(s) for s in w["score"][:2]] == [-7.5, -7.5] and [float(s) for s in w["token_logprob"][:2]] == [0.0, 0.0]
    assert w["token"].tolist()[2:] == [1, 49, 50] and w["ended"].tolist()[2:] == [0, 1, 0]
    w = bc.reference("all_ended_w5")
    assert w["parent"].tolist() == [3, 0, 1, 2, 4] and w["token"].tolist() == [44, 11, 22, 33, V - 1] and w["ended"].tolist() == [1] * 5
    # one beam far ahead, and the shape of step 0: every winner from one row, in the row's own order
    assert bc.reference("ahead_w5")["parent"].tolist() == [1] * 5
    for name in ("step0_w5", "step0_w16"):
        w = bc.reference(name, 1)
        assert w["parent"].tolist() == [1] * bc.width(name) and np.all(np.diff(w["score"].astype(np.float64)) < 0)


def test_pruning_loses_nothing():
    """every winner of the brute-force reference is among its row's top W + 1 without id 0 (or is an ended row's token)"""
    for name, r in bc.case_shifts():
        rows, cum, ended, last, stops = bc.shifted(name, r)
        W, want = len(rows), bc.reference(name, r)
        ids, _ = bc.rows_topn(rows, W + 1)
        for p, t in zip(want["parent"].tolist(), want["token"].tolist()):
            assert (t == last[p]) if ended[p] else (t != 0 and t in ids[p].tolist()), (name, r, p, t)
