"""Log-probs and top-n alternatives on the device (csrc/topn.hip.h: k_topn_part, k_topn_finish; rwkv_topn_rows / rwkv_decode_batch_logprobs).
Planted rows (tests/logprob_cases.py) at all four row alignments against the numpy f64 reference: ids equal, |d logprob| <= 1e-10, -inf exactly
-inf, and every log-prob bitwise that of rwkv_score_rows.  The device loops against the caller's loop they stand for -- forward, score_rows,
topn_rows per step -- bitwise, and against rwkv_decode_batch_until for ids, lengths, reasons and final slots; stops, budgets and a KEEP
continuation; rejected calls; scratch accounting; the C++ and pybind bindings.  Every context is a synthetic 2-layer model.
Each planted case prints its worst figure before anything is asserted."""
import ctypes as C

import numpy as np
import pytest

import logprob_cases as lc
import support
from support import E_ARG, E_STATE, V, build_app, eng, firsts_of, load, restore, run_app, rwkv_mod, same_bits, seeds_of, slots, start_state  # noqa: F401

from rwkv_cpp_accelerated_amd import modelfile as mf

pytestmark = pytest.mark.gpu

L = 2
ROWS = 4                         # maxGPT of the planted context: rows 0 .. 3 start at the four offsets from a 16-byte boundary
D_LOOP, MAXN, STEPS = 128, 5, 12
NUC = dict(temp=1.0, top_p=0.9, presence=0.4, frequency=0.4, decay=0.996)      # nucleus with penalties: the counts are part of a slot
KW = dict(greedy=dict(pick="greedy"), nucleus=dict(pick="nucleus", **NUC))


@pytest.fixture(scope="module")
def planted(eng):
    m = load(eng, L, 64, 3, ROWS)
    m.forward(5)
    yield m
    m.close()


@pytest.fixture(scope="module")
def model(eng):
    m = load(eng, L, D_LOOP, 41, MAXN, head_scale=30.0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def start(eng, model):
    """distinct state in every slot: where every run of the loop tests starts"""
    return start_state(eng, model, MAXN)


def plant(m, rows):
    """rows: {logits row: case name}"""
    support.plant_rows(m, {r: lc.logits_of(name) for r, name in rows.items()}, ROWS)


# ---- planted rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lc.CASES)
def test_planted_case_on_each_of_the_four_row_alignments(planted, name):
    m = planted
    plant(m, {r: name for r in range(ROWS)})
    before = m.logits(ROWS).copy()
    want_ids, want_lp = lc.ref_of(name)
    bad, worst = [], 0.0
    for n in lc.TOP_NS:
        ids, lp = m.topn_rows(list(range(ROWS)), n)
        assert ids.shape == (ROWS, n) and lp.shape == (ROWS, n) and ids.min() >= 0 and ids.max() < V
        w, b = lc.check(f"{name} n={n}", ids, lp, np.tile(want_ids[:n], (ROWS, 1)), np.tile(want_lp[:n], (ROWS, 1)))
        worst, bad = max(worst, w), bad + b
        s_lp, _, _ = m.score_rows([r for r in range(ROWS) for _ in range(n)], ids.reshape(-1).tolist())
        if not same_bits(s_lp, lp.reshape(-1)):
            bad.append(f"{name} n={n}: top log-probs are not the bits of score_rows")
    print(f"{name:>14}: worst |d logprob| {worst:.2e}  top-5 {ids[0][:5].tolist()}  -inf entries at n=32: {int(np.isneginf(lp[0]).sum())}")
    assert not bad, bad
    assert same_bits(before, m.logits(ROWS))                                            # the top-n leaves the logits alone


def test_one_call_repeats_rows_out_of_order_across_different_cases(planted):
    m = planted
    held = {0: "one_thread", 1: "neginf", 2: "straddle", 3: "wide"}
    plant(m, held)
    rows = [3, 0, 3, 2, 1, 1, 0, 3, 2, 0]
    for n in (5, 32):
        ids, lp = m.topn_rows(rows, n)
        w, bad = lc.check(f"mixed n={n}", ids, lp, [lc.ref_of(held[r])[0][:n] for r in rows], [lc.ref_of(held[r])[1][:n] for r in rows])
        print(f"         mixed: n {n} queries {len(rows)}  worst |d logprob| {w:.2e}")
        assert not bad, bad


def test_rows_after_a_parralel_step(eng, model, start):
    m = model
    restore(m, start)
    lg = m.forward([5, 40000, 77], eng.MODE_PARRALEL)[: 3 * V].reshape(3, V).copy()
    rows = [2, 0, 1, 0]
    ids, lp = m.topn_rows(rows, 20)
    refs = [lc.topn_reference(lg[r], 20) for r in rows]
    w, bad = lc.check("parralel", ids, lp, [r[0] for r in refs], [r[1] for r in refs])
    print(f"      parralel: worst |d logprob| {w:.2e}")
    assert not bad, bad


# ---- the loops against the caller's loop they stand for -------------------------------------------------------------------------
def callers_loop(eng, m, first, picks, top_n):
    """what a caller does today: per step one forward of the ids fed at that step, then score_rows of the picks and topn_rows, rows 0 .. N - 1"""
    n, steps = picks.shape
    lp, ent = np.zeros((n, steps)), np.zeros((n, steps))
    tid, tlp = np.zeros((n, steps, top_n), np.int64), np.zeros((n, steps, top_n))
    fed = list(first)
    for k in range(steps):
        if n == 1:
            m.forward(int(fed[0]))
        else:
            m.forward([int(t) for t in fed], eng.MODE_PARRALEL)
        lp[:, k], ent[:, k], _ = m.score_rows(list(range(n)), picks[:, k].tolist())
        if top_n:
            tid[:, k], tlp[:, k] = m.topn_rows(list(range(n)), top_n)
        fed = picks[:, k].tolist()
    return lp, ent, tid, tlp


@pytest.mark.parametrize("top_n", [0, 5, 32])
@pytest.mark.parametrize("kind", ["greedy", "nucleus"])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_the_record_is_the_callers_loop_and_the_run_is_the_until_call(eng, model, start, n, kind, top_n):
    m, first, seeds = model, firsts_of(n), seeds_of(n)
    restore(m, start)
    ids, ln, rs, ran, lp, ent, tid, tlp = m.decode_batch_logprobs(first, STEPS, top_n=top_n, seeds=seeds, **KW[kind])
    got = slots(m, n, kind == "nucleus")
    assert tid.shape == (n, STEPS, top_n) and tlp.shape == (n, STEPS, top_n) and lp.shape == (n, STEPS) and ent.shape == (n, STEPS)
    # ids, lengths, reasons and the final slots are those of the until call with the same arguments
    restore(m, start)
    u_ids, u_ln, u_rs, u_ran = m.decode_batch_until(first, STEPS, seeds=seeds, **KW[kind])
    ref = slots(m, n, kind == "nucleus")
    assert np.array_equal(ids, u_ids) and np.array_equal(ln, u_ln) and np.array_equal(rs, u_rs) and ran == u_ran == STEPS
    for g, r in zip(got, ref):
        assert same_bits(g, r)
    # the record, bit for bit, is what the caller's loop computes
    restore(m, start)
    w_lp, w_ent, w_tid, w_tlp = callers_loop(eng, m, first, ids.astype(np.int64), top_n)
    assert same_bits(lp, w_lp) and same_bits(ent, w_ent)
    assert np.array_equal(tid, w_tid) and same_bits(tlp, w_tlp)
    assert np.isfinite(lp).all() and (lp <= 0).all() and np.isfinite(ent).all()
    if top_n:
        assert (tlp[:, :, 0] >= lp).all()                                                # no pick is more probable than the most probable token
        if kind == "greedy":                                                             # the greedy pick is the top-1 unless that is the banned id 0
            assert ((tid[:, :, 0] == ids) | (tid[:, :, 0] == 0)).all()
    # entropy = False leaves the entropies out, and changes nothing else
    restore(m, start)
    again = m.decode_batch_logprobs(first, STEPS, top_n=top_n, entropy=False, seeds=seeds, **KW[kind])
    assert again[5] is None and np.array_equal(again[0], ids) and same_bits(again[4], lp) and same_bits(again[7], tlp)


# ---- with stops ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["greedy", "nucleus"])
def test_stops_and_budgets_cut_the_record_where_they_cut_the_ids(eng, model, start, kind):
    m, n, top_n = model, 5, 5
    first, seeds, budgets = firsts_of(n), seeds_of(n), [3, 12, 7, 1, 12]
    restore(m, start)
    full = m.decode_batch_logprobs(first, STEPS, top_n=top_n, seeds=seeds, **KW[kind])
    stop = [int(v) for v in full[0][1][5:7]]                                             # stream 1 spells it at steps 5, 6 (if not earlier)
    restore(m, start)
    ids, ln, rs, ran, lp, ent, tid, tlp = m.decode_batch_logprobs(first, STEPS, top_n=top_n, seeds=seeds, stops=[stop], max_new=budgets, **KW[kind])
    got = slots(m, n, kind == "nucleus")
    restore(m, start)
    u = m.decode_batch_until(first, STEPS, seeds=seeds, stops=[stop], max_new=budgets, **KW[kind])
    ref = slots(m, n, kind == "nucleus")
    assert np.array_equal(ids, u[0]) and np.array_equal(ln, u[1]) and np.array_equal(rs, u[2]) and ran == u[3]
    for g, r in zip(got, ref):
        assert same_bits(g, r)
    print(f"{kind}: len {ln.tolist()} reason {rs.tolist()} steps_run {ran}")
    assert ln[0] == 3 and ln[3] == 1 and ln[2] <= 7 and ln[1] <= 7 and rs[1] == 2
    for s in range(n):
        k = int(ln[s])
        for a, b in zip((lp, ent, tid, tlp), full[4:]):
            assert same_bits(a[s, :k], b[s, :k]), s                                      # below the length: the record of the run without stops
            assert not a[s, k:].any(), s                                                 # from it on: 0 / 0.0


def test_a_keep_continuation_gives_the_record_of_the_one_call(eng, model, start):
    m, n, top_n = model, 5, 5
    first, seeds = firsts_of(n), seeds_of(n)
    restore(m, start)
    plain = m.decode_batch_logprobs(first, 16, top_n=top_n, seeds=seeds, **KW["nucleus"])
    stop = [int(plain[0][0][7]), int(plain[0][0][8])]                                    # stream 0 spells it across the split
    restore(m, start)
    full = m.decode_batch_logprobs(first, 16, top_n=top_n, seeds=seeds, stops=[stop], **KW["nucleus"])
    restore(m, start)
    a = m.decode_batch_logprobs(first, 8, top_n=top_n, seeds=seeds, stops=[stop], **KW["nucleus"])
    b = m.decode_batch_logprobs(a[0][:, 7].tolist(), 8, top_n=top_n, seeds=[s + 8 for s in seeds], stops=[stop], keep=True, **KW["nucleus"])
    assert full[1][0] <= 9
    checked = 0
    for s in range(n):
        if a[1][s] < 8:                                                                  # (stopped inside the first call: nothing to continue)
            continue
        k2 = int(b[1][s])
        assert full[1][s] == 8 + k2 and full[2][s] == b[2][s], s
        for i in (0, 4, 5, 6, 7):
            assert same_bits(np.concatenate([a[i][s], b[i][s][:k2]]), full[i][s][: 8 + k2]), (s, i)
        checked += 1
    assert checked >= 3


# ---- rejected calls -----------------------------------------------------------------------------------------------------------
def test_rejected_calls_leave_everything_alone(eng, model, start):
    lib, m = eng.lib(), model
    u64, u32, dbl = C.c_uint64, C.c_uint32, C.c_double
    restore(m, start)
    m.decode_batch_logprobs(firsts_of(2), 4, top_n=3)
    state, resident = slots(m, MAXN, False), m.resident_bytes()
    a = lambda *v: (u64 * len(v))(*v)
    n, steps = 2, 4
    lp, ent, tid, tlp = (dbl * 64)(), (dbl * 64)(), (u64 * 64 * 33)(), (dbl * 64 * 33)()
    out, ln, rs, ran = (u64 * 64)(), (u32 * 8)(), (u32 * 8)(), u64(0)
    greedy = eng.Pick(eng.PICK_GREEDY, 1.0, 0.8, 0, eng.nucleus_params())
    sp, alive = eng.stop_params([[5, 6]], [4, 4])
    dp, up = C.POINTER(dbl), C.POINTER(u64)
    cast = lambda x, t: None if x is None else C.cast(x, t)

    def rec(top_n=3, reserved=0, logprob=lp, entropy=ent, top_ids=tid, top_logprob=tlp):
        return eng.LogprobOut(top_n, reserved, cast(logprob, dp), cast(entropy, dp), cast(top_ids, up), cast(top_logprob, dp))

    def call(r=None, h=m._h, first=a(5, 6), n=n, steps=steps, pick=greedy, seeds=None, stop=sp, out=out, ln=ln, null_rec=False):
        r = rec() if r is None else r
        return int(lib.rwkv_decode_batch_logprobs(h, first, n, steps, None if pick is None else C.byref(pick), seeds, None if stop is None else C.byref(stop),
                                                  None if null_rec else C.byref(r), out, ln, rs, C.byref(ran)))

    assert call(null_rec=True) == E_ARG
    assert call(rec(logprob=None)) == E_ARG
    assert call(rec(top_n=33)) == E_ARG
    assert call(rec(top_n=3, top_ids=None)) == E_ARG and call(rec(top_n=3, top_logprob=None)) == E_ARG
    assert call(rec(top_n=0)) == E_ARG                                       # top_ids / top_logprob given with top_n == 0
    assert call(rec(top_n=0, top_ids=None)) == E_ARG and call(rec(top_n=0, top_logprob=None)) == E_ARG
    assert call(rec(reserved=1)) == E_ARG
    assert call(ln=None) == E_ARG                                            # a stop without out_len
    assert call(pick=None) == E_ARG and call(first=None) == E_ARG and call(out=None) == E_ARG
    # whatever the until call rejects
    assert call(n=0) == E_ARG and call(n=MAXN + 1) == E_ARG and call(steps=0) == E_ARG and call(steps=65537) == E_ARG
    assert call(first=a(5, V)) == E_ARG
    assert call(pick=eng.Pick(7, 1.0, 0.8, 0, eng.nucleus_params())) == E_ARG
    assert call(pick=eng.Pick(eng.PICK_NUCLEUS, 1.0, 0.8, 0, eng.nucleus_params()), seeds=None) == E_ARG       # sampled without seeds
    assert call(pick=eng.Pick(eng.PICK_NUCLEUS, 1.0, 0.8, 0, eng.nucleus_params(temp=0.0)), seeds=a(1, 2)) == E_ARG
    bad_stop, alive2 = eng.stop_params([[5] * 9], None)
    assert call(stop=bad_stop) == E_ARG
    bad_budget, alive3 = eng.stop_params([], [4, 5])
    assert call(stop=bad_budget) == E_ARG
    # the entries bound: 2 x 65536 x 33 > 2^22, checked before anything is allocated (the arrays are never written)
    assert 2 * 65536 * 33 > eng.LOGPROB_ENTRIES_MAX
    assert call(rec(top_n=32), steps=65536, stop=None) == E_ARG
    for x, y in zip(state, slots(m, MAXN, False)):
        assert same_bits(x, y)
    assert m.resident_bytes() == resident
    # rwkv_topn_rows
    T = lambda rows, cnt, top_n, i=tid, l=tlp, h=m._h: int(lib.rwkv_topn_rows(h, rows, cnt, top_n, cast(i, up), cast(l, dp)))
    assert T(a(0, MAXN), 2, 3) == E_ARG                                      # a row = max_ctx
    assert T(a(0, 1), 0, 3) == E_ARG and T(a(0, 1), 65537, 3) == E_ARG
    assert T(a(0, 1), 2, 0) == E_ARG and T(a(0, 1), 2, 33) == E_ARG
    assert T(None, 2, 3) == E_ARG and T(a(0, 1), 2, 3, None) == E_ARG and T(a(0, 1), 2, 3, tid, None) == E_ARG
    for x, y in zip(state, slots(m, MAXN, False)):
        assert same_bits(x, y)
    assert m.resident_bytes() == resident
    # accepted: NULL stop with NULL out_len and reason; NULL entropy
    assert call(rec(entropy=None), stop=None, ln=None) == 0 and call() == 0 and T(a(1, 0), 2, 3) == 0
    del alive, alive2, alive3
    # not loaded
    e = eng.RWKV(resident=True)
    assert call(h=e._h) == E_STATE and T(a(0), 1, 1, h=e._h) == E_STATE
    assert call(h=e._h, null_rec=True) == E_ARG and T(None, 1, 1, h=e._h) == E_ARG
    e.close()
    # pipeline stages: no stage runs the loop; the last one holds a head and its rows (zeros: the uniform distribution, ids 0 .. n - 1)
    t = mf.synthetic_tensors(L, 64, seed=3)
    for (l0, l1, status) in ((0, 1, E_STATE), (1, 2, 0)):
        e = eng.RWKV(resident=True)
        e.set_layer_range(l0, l1)
        e.loadTensors(L, 64, t, maxGPT=2)
        assert T(a(1), 1, 3, h=e._h) == status
        if status == 0:
            assert [int(tid[0][j]) for j in range(3)] == [0, 1, 2] and abs(tlp[0][0] + np.log(V)) < 1e-10
        assert call(h=e._h) == E_STATE
        e.close()
    # a context without the chunk path runs one stream only
    e = load(eng, L, 48, 42, 3)
    assert call(h=e._h, stop=None) == E_STATE and call(h=e._h, first=a(5), n=1, stop=None) == 0
    e.close()


# ---- scratch accounting -------------------------------------------------------------------------------------------------------
def record_bytes(n, steps, top_n):
    """LP_REC of include/rwkv_mi355x.h: per stream 8 + 128 (4 + top_n) bytes of scratch, per stream and step 16 (1 + top_n)"""
    return n * (8 + 128 * (4 + top_n)) + n * steps * 16 * (1 + top_n)


def test_the_record_is_counted_and_a_plain_until_call_allocates_what_it_did(eng):
    D, n = 64, 4
    park = 4 * n * (10 * L * D + 50280) + 4 * (5 * n + 2) + 4 * 8 * 8        # park buffer, run record, histories (tests/test_stop_gpu.py)
    m = load(eng, L, D, 9, 8)
    m.decode_batch_until(firsts_of(n), 9)                                    # cannot stop a stream: the plain loop (9 steps: the ids of the longest call below)
    base = m.resident_bytes()
    m.decode_batch_until(firsts_of(n), 8, max_new=[8] * n)
    assert m.resident_bytes() - base == park                                 # before any logprobs call: what it did
    r0 = m.resident_bytes()
    m.decode_batch_logprobs(firsts_of(n), 8, top_n=5)
    r1 = m.resident_bytes()
    assert r1 - r0 == record_bytes(n, 8, 5)
    m.decode_batch_logprobs(firsts_of(n - 1), 6, top_n=5, max_new=[6] * (n - 1))
    m.topn_rows([0, 1], 5)
    assert m.resident_bytes() == r1                                          # smaller calls fit
    m.decode_batch_logprobs(firsts_of(n), 9, top_n=5)
    assert m.resident_bytes() - r0 == record_bytes(n, 9, 5)
    m.close()
    m = load(eng, L, D, 9, 8)                                                # the other order: the record first
    m.decode_batch_greedy(firsts_of(n), 8)
    base = m.resident_bytes()
    m.decode_batch_logprobs(firsts_of(n), 8, top_n=0)
    assert m.resident_bytes() - base == record_bytes(n, 8, 0)
    r0 = m.resident_bytes()
    m.decode_batch_until(firsts_of(n), 8, max_new=[8] * n)
    assert m.resident_bytes() - r0 == park
    m.close()


# ---- bindings -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_file(tmp_path_factory):
    return support.model_file(tmp_path_factory, "logprobs", L, D_LOOP, 43, head_scale=30.0)


def test_logprobs_app_matches_the_python_engine(eng, built, model_file, tmp_path):
    n, steps, top_n = 3, 6, 4
    rc, lines, raw = run_app(build_app("logprobs_app", tmp_path), [model_file, n, steps, top_n])
    assert rc == 0, raw
    lines = [l.split() for l in lines]
    assert lines[-1] == ["logprobs_ok"] and len(lines) == n * steps + n + 1
    m = eng.RWKV(resident=True)
    m.loadFile(model_file, n)
    m.forward([5, 6, 7], eng.MODE_GPT)
    for s in range(1, n):
        m.copy_state(s, 0)
    ids, ln, rs, ran, lp, ent, tid, tlp = m.decode_batch_logprobs([100 + s for s in range(n)], steps, top_n=top_n, seeds=list(range(n)), **KW["nucleus"])
    r_ids, r_lp = m.topn_rows(list(range(n)), top_n)
    m.close()
    hx = float.fromhex
    for f in lines[: n * steps]:
        s, k = int(f[0]), int(f[1])
        assert int(f[2]) == ids[s, k] and hx(f[3]).hex() == float(lp[s, k]).hex() and hx(f[4]).hex() == float(ent[s, k]).hex(), (s, k)
        assert [int(v) for v in f[5::2]] == tid[s, k].tolist() and [hx(v).hex() for v in f[6::2]] == [float(v).hex() for v in tlp[s, k]], (s, k)
    for f in lines[n * steps:-1]:
        s = int(f[1])
        assert f[0] == "row" and [int(v) for v in f[2::2]] == r_ids[s].tolist() and [hx(v).hex() for v in f[3::2]] == [float(v).hex() for v in r_lp[s]]


def test_pybind_top_logprobs_matches_the_python_engine(eng, rwkv_mod, model_file):
    rwkv = rwkv_mod
    h = rwkv.initRwkv()
    rwkv.loadModel(h, model_file)
    rwkv.initOutput(h); rwkv.initState(h)
    rwkv.modelForward(h, 1234)
    got_ids, got_lp = rwkv.topLogprobs(h, [0, 0], 7)
    rwkv.freeRwkv(h)
    m = eng.RWKV(resident=True)
    m.loadFile(model_file)                           # maxGPT 1, as loadModel
    m.forward(1234)
    ids, lp = m.topn_rows([0, 0], 7)
    m.close()
    assert got_ids.shape == (2, 7) and got_lp.dtype == np.float64 and np.array_equal(got_ids, ids) and same_bits(np.asarray(got_lp), lp)
    assert np.isfinite(lp).all() and (np.diff(lp, axis=1) <= 0).all()
