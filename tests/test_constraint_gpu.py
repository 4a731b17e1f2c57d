"""Constrained decoding on the device (csrc/constrain.hip.h: k_constraint_mask, k_constrain_rows, k_constraint_advance; rwkv_pick_constrained /
rwkv_decode_batch_constrained).  Planted rows (tests/constraint_cases.py) at all four row alignments: the second buffer bit for bit the numpy
row, the greedy pick numpy's argmax, the nucleus pick bit for bit what rwkv_sample_nucleus draws from the same numbers planted as logits, the
advance, the logits untouched.  The device loops bit for bit against the caller's loop they replace (forward, host mask, upload, sample_nucleus,
host advance), against rwkv_decode_batch_until under an allow-everything automaton, a trie of four choices (reason 32, park / unpark, precedence),
a KEEP continuation, the log-prob hook, rejected calls, accounting and the C++ / pybind bindings.  Every context is a synthetic 2-layer model.
No tolerance anywhere: the constrained pick is the existing pick on the same numbers."""
import ctypes as C

import numpy as np
import pytest

import constraint_cases as cc
import sampler_cases
import support
from support import E_ARG, E_STATE, V, build_app, eng, firsts_of, load, plant_rows, restore, run_app, rwkv_mod, same_bits, seeds_of, slots, start_state  # noqa: F401

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
    m.constraint_set(*cc.planted_automaton())
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


# ---- planted rows through rwkv_pick_constrained -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.PLANTED_STATES))
def test_greedy_pick_on_each_of_the_four_row_alignments(planted, name):
    m, a, q = planted, cc.planted_automaton(), cc.PLANTED_STATES[name]
    mask = cc.allowed_mask(a, q)
    rows = {r: cc.planted_row(mask, 10 * q + r) for r in range(ROWS)}
    plant_rows(m, rows, ROWS)
    m.constraint_state_set([q] * ROWS)
    before = m.logits(ROWS).copy()
    for r in range(ROWS):
        want = cc.constrained(rows[r], mask)
        g, state = m.pick_constrained("greedy", row=r, slot=r, advance=False)
        got = m.debug_constrained_row(r)
        print(f"{name:>11} row {r}: pick {g} (numpy {cc.argmax_low(want)}), {int(mask.sum())} ids allowed, best masked logit {rows[r][~mask].max():.1f}")
        assert same_bits(got, want), (name, r)                                              # the second buffer, padding excluded: the row itself
        assert g == cc.argmax_low(want) and mask[g] and state == q
    assert same_bits(before, m.logits(ROWS)) and m.constraint_state_get().tolist() == [q] * ROWS


def test_bias_cases(planted):
    m, a = planted, cc.planted_automaton()
    every, triple = cc.allowed_mask(a, cc.P_ALL), cc.allowed_mask(a, cc.P_TRIPLE)
    rows = {r: cc.planted_row(triple, 77 + r) for r in range(ROWS)}                         # the best of 31, 32, 33 lies 50 below every other id
    plant_rows(m, rows, ROWS)
    before = m.logits(ROWS).copy()
    for r in range(ROWS):
        l = rows[r]
        order = [int(i) for i in np.argsort(-cc.constrained(l, triple), kind="stable")[:3]]           # winner, second, third of the triple
        gap = float(l[order[0]] - l[order[2]])
        cases = [
            (cc.P_ALL, every, {1: 500.0, V - 1: 400.0}, 1),                                 # a bias on id 1 and on 50276
            (cc.P_ALL, every, {1: 400.0, V - 1: 500.0}, V - 1),
            (cc.P_TRIPLE, triple, {order[0]: -np.inf}, order[1]),                           # -inf on the otherwise winning allowed id
            (cc.P_TRIPLE, triple, {100: 1000.0, 20000: -np.inf}, order[0]),                 # a bias on masked ids changes nothing
            (cc.P_TRIPLE, triple, {order[2]: gap + 1.0}, order[2]),                         # a bias that changes the winner
            (cc.P_TRIPLE, triple, {}, order[0]),
        ]
        for q, mask, bias, winner in cases:
            m.constraint_state_set([q], slot0=r)
            want = cc.constrained(l, mask, bias)
            g, _ = m.pick_constrained("greedy", bias=bias, row=r, slot=r, advance=False)
            assert same_bits(m.debug_constrained_row(r), want), (r, bias)
            assert g == cc.argmax_low(want) == winner, (r, bias, g)
        assert same_bits(cc.constrained(l, triple, {100: 1000.0, 20000: -np.inf}), cc.constrained(l, triple))
    assert same_bits(before, m.logits(ROWS))


@pytest.mark.parametrize("penalty", [False, True])
@pytest.mark.parametrize("name", list(cc.PLANTED_STATES))
def test_nucleus_pick_is_sample_nucleus_on_the_planted_constrained_row(planted, name, penalty):
    m, a, q = planted, cc.planted_automaton(), cc.PLANTED_STATES[name]
    mask = cc.allowed_mask(a, q)
    ids = np.flatnonzero(mask)
    bias = {int(ids[0]): -0.75, int(ids[-1]): 1.5}
    kw = dict(temp=0.8, top_p=0.95, presence=0.4 if penalty else 0.0, frequency=0.3 if penalty else 0.0, decay=0.99)
    rows = {r: cc.planted_row(mask, 200 + 10 * q + r) for r in range(ROWS)}
    counts = np.zeros(V, np.float32)
    counts[ids[:: max(1, len(ids) // 7)]] = np.float32(1.75)                                # some allowed ids have been seen
    m.constraint_state_set([q] * ROWS)
    for r in range(ROWS):
        m.penalty_set(r, counts if penalty else None)
    for r in range(ROWS):
        c = cc.constrained(rows[r], mask, bias)
        plant_rows(m, {r: c}, ROWS)                                                         # the existing kernel on the same numbers ...
        ref = [m.sample_nucleus(u=u, row=r, slot=r, ban0=False, **kw) for u in (0.0, 0.25, 0.5, 0.999999)]
        plant_rows(m, {r: rows[r]}, ROWS)                                                   # ... and the model's row back
        got = [m.pick_constrained("nucleus", bias=bias, u=u, row=r, slot=r, advance=False, **kw)[0] for u in (0.0, 0.25, 0.5, 0.999999)]
        print(f"{name:>11} row {r} penalty {penalty}: {got}")
        assert got == ref and all(mask[g] for g in got), (name, r, got, ref)
        assert same_bits(m.debug_constrained_row(r), c) and same_bits(m.logits(ROWS).reshape(ROWS, V)[r], rows[r])
        assert same_bits(m.penalty_get(r), counts if penalty else np.zeros(V, np.float32))  # no update without the flag


def test_advance(planted):
    m, a = planted, cc.planted_automaton()
    every = cc.allowed_mask(a, cc.P_ALL)
    for q, g, want in ((cc.P_TRIPLE, 31, 3), (cc.P_TRIPLE, 33, 5), (cc.P_TRIPLE2, 31, 6), (cc.P_TRIPLE2, 33, 1), (cc.P_ONE, 1, 1),
                       (cc.P_TAIL, 50272, 0), (cc.P_LAST, V - 1, 2), (cc.P_ALL, V - 1, (V - 1) % 6)):
        assert cc.next_state(a, q, g) == want
        l = np.zeros(V, np.float32)
        l[g] = 9.0                                                                          # the winner among whatever q allows
        for r in (0, 3):
            plant_rows(m, {r: l}, ROWS)
            m.constraint_state_set([q] * ROWS)
            assert m.pick_constrained("greedy", row=r, slot=r, advance=False) == (g, q)
            assert m.constraint_state_get().tolist() == [q] * ROWS                          # advance = 0 leaves q alone
            assert m.pick_constrained("greedy", row=r, slot=r, advance=True) == (g, want)
            exp = [q] * ROWS
            exp[r] = want
            assert m.constraint_state_get().tolist() == exp                                 # only this slot moved
    assert every.sum() == V - 1


# ---- the loops against the caller's loop they replace -----------------------------------------------------------------------------
def callers_loop(eng, m, a, first, seeds, kind, steps, start_q, bias=None):
    """what a caller does today, per step: forward; the numpy constrained row; plant it; sample_nucleus (or numpy argmax) per row; the
    advance on the host; feed.  Returns ids [n][steps], q [n], the model's logits rows of the last step, and the log-probs of the picks under
    the MODEL's rows (score_rows, in front of the planting)"""
    n = len(first)
    ids, lp = np.zeros((n, steps), np.int64), np.zeros((n, steps))
    q, fed = list(start_q), list(first)
    if kind == "nucleus":
        for s in range(n):
            m.penalty_set(s, None)
    for k in range(steps):
        if n == 1:
            m.forward(int(fed[0]))
        else:
            m.forward([int(t) for t in fed], eng.MODE_PARRALEL)
        rows = m.logits(n).reshape(n, V).copy()
        c = [cc.constrained(rows[s], cc.allowed_mask(a, q[s]), bias[s] if bias else None) for s in range(n)]
        if kind == "nucleus":
            plant_rows(m, {s: c[s] for s in range(n)}, MAXN)
            for s in range(n):
                u = sampler_cases.splitmix_u(seeds[s], k)
                ids[s, k] = m.sample_nucleus(u=u, row=s, slot=s, ban0=False, update=True, **NUC)
            plant_rows(m, {s: rows[s] for s in range(n)}, MAXN)
        else:
            ids[:, k] = [cc.argmax_low(c[s]) for s in range(n)]
        lp[:, k], _, _ = m.score_rows(list(range(n)), ids[:, k].tolist())
        q = [cc.next_state(a, q[s], int(ids[s, k])) for s in range(n)]
        fed = ids[:, k].tolist()
    return ids, q, rows, lp


@pytest.mark.parametrize("kind", ["greedy", "nucleus"])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_the_loop_is_the_callers_loop_it_replaces(eng, model, start, n, kind):
    m, a = model, cc.loop_automaton()
    first, seeds = firsts_of(n), seeds_of(n)
    q0 = [s % 6 for s in range(n)]
    bias = [{int(a[1][a[0][q0[s]]]): -np.inf, 7 + s: 3.0} for s in range(n)]               # ban the lowest id the start state allows
    m.constraint_set(*a)
    restore(m, start)
    w_ids, w_q, w_rows, w_lp = callers_loop(eng, m, a, first, seeds, kind, STEPS, q0, bias)
    want = slots(m, n, kind == "nucleus")
    restore(m, start)
    ids, ln, rs, ran, q, lp, ent, tid, tlp = m.decode_batch_constrained(first, STEPS, start=q0, bias=bias, logprobs=True, seeds=seeds, **KW[kind])
    got = slots(m, n, kind == "nucleus")
    print(f"{kind} n={n}: ids[0] {ids[0].tolist()} q {q.tolist()}")
    assert np.array_equal(ids, w_ids) and q.tolist() == w_q == m.constraint_state_get(0, n).tolist()
    assert ln.tolist() == [STEPS] * n and rs.tolist() == [0] * n and ran == STEPS
    for s in range(n):                                                                      # every pick is an id its state allowed
        qs = q0[s]
        for k in range(STEPS):
            assert cc.allowed_mask(a, qs)[ids[s, k]] and not (k == 0 and ids[s, k] == a[1][a[0][q0[s]]])
            qs = cc.next_state(a, qs, int(ids[s, k]))
    for g, w in zip(got, want):
        assert same_bits(g, w)                                                              # the five state arrays, the logits rows, the counts
    assert same_bits(got[5], w_rows)                                                        # the last step's rows are the MODEL's
    assert same_bits(lp, w_lp)                                                              # and so are the recorded log-probs: nothing of the mask shows
    m.constraint_clear()


@pytest.mark.parametrize("logprobs", [False, True])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("kind", ["greedy", "nucleus"])
def test_an_allow_everything_automaton_is_the_until_call(eng, model, start, kind, n, logprobs):
    """stops, budgets, the constraint and (logprobs) the record in one call, in the one-stream form and the batched one: the only place
    where every hook of the decode loops is on at once"""
    m = model
    first, seeds, budgets = firsts_of(n), seeds_of(n), [3, 12, 7, 1, 12] if n == 5 else [7]
    restore(m, start)
    full = m.decode_batch_until(first, STEPS, seeds=seeds, **KW[kind])
    stop = [int(v) for v in (full[0][1][5:7] if n == 5 else full[0][0][3:5])]               # n = 1: the stream's own ids, complete at step 5 of 12
    rec = dict(logprobs=True, top_n=3) if logprobs else {}
    restore(m, start)
    if logprobs:
        u = m.decode_batch_logprobs(first, STEPS, top_n=3, seeds=seeds, stops=[stop], max_new=budgets, **KW[kind])
    else:
        u = m.decode_batch_until(first, STEPS, seeds=seeds, stops=[stop], max_new=budgets, **KW[kind])
    ref = slots(m, n, kind == "nucleus")
    if n == 1:
        assert u[1][0] <= 5 and u[2][0] == 2                                          # the stop fired in mid-run, in front of the budget
    m.constraint_set(*cc.everything_automaton())
    restore(m, start)
    r = m.decode_batch_constrained(first, STEPS, seeds=seeds, stops=[stop], max_new=budgets, **rec, **KW[kind])
    got = slots(m, n, kind == "nucleus")
    m.constraint_clear()
    restore(m, start)
    b = m.decode_batch_constrained(first, STEPS, seeds=seeds, stops=[stop], max_new=budgets, **rec, **KW[kind])     # no automaton: the implicit state
    if not np.array_equal(r[0], u[0]):
        print(f"{kind} n={n} logprobs={logprobs}: len {u[1].tolist()} reason {u[2].tolist()} steps_run {u[3]}")
        print("row maxima of the last step:", ref[5].max(axis=1))                           # (-inf instead of -99 at id 0 can only show at a tiny logit scale)
    assert np.array_equal(r[0], u[0]) and np.array_equal(b[0], u[0])
    assert np.array_equal(r[1], u[1]) and np.array_equal(r[2], u[2]) and r[3] == u[3] and r[4].tolist() == [0] * n
    assert np.array_equal(b[1], u[1]) and np.array_equal(b[2], u[2])
    for g, w in zip(got, ref):
        assert same_bits(g, w)
    for i in range(4, len(u)):                                                              # logprob, entropy, top_ids, top_logprob: the MODEL's, bit for bit
        assert same_bits(r[i + 1], u[i]) and same_bits(b[i + 1], u[i])


def test_a_trie_of_four_choices(eng, model, start):
    m, n, steps = model, 5, 24
    a = eng.constraint_trie(cc.CHOICES)
    first, seeds = firsts_of(n), seeds_of(n)
    m.constraint_set(*a)
    restore(m, start)
    ids, ln, rs, ran, q = m.decode_batch_constrained(first, steps, start=[0] * n, seeds=seeds, **KW["nucleus"])
    got = slots(m, n, True)
    print(f"trie: len {ln.tolist()} reason {rs.tolist()} q {q.tolist()} steps_run {ran}")
    spelled = []
    for s in range(n):
        seq = ids[s, : ln[s]].tolist()
        assert seq in cc.CHOICES and cc.trie_accepts(a, seq) and not ids[s, ln[s]:].any(), (s, seq)
        assert rs[s] == eng.STOP_CONSTRAINT and a[0][q[s]] == a[0][q[s] + 1]                # ended by the automaton, on that leaf
        qq = 0
        for g in seq:
            qq = cc.next_state(a, qq, g)
        assert qq == q[s]
        spelled.append(seq)
    assert ran <= min(steps, 8 * ((int(ln.max()) - 1) // 8 + 2)) and m.constraint_state_get(0, n).tolist() == q.tolist()
    # each slot is bit for bit the slot of the same call cut at out_len[s]: the park / unpark path
    for cut in sorted(set(ln.tolist())):
        restore(m, start)
        c_ids, c_ln, c_rs, _, c_q = m.decode_batch_constrained(first, cut, start=[0] * n, seeds=seeds, **KW["nucleus"])
        ref = slots(m, n, True)
        for s in range(n):
            if ln[s] == cut:
                assert c_ln[s] == cut and c_rs[s] == eng.STOP_CONSTRAINT and c_q[s] == q[s]     # reported at the call's last step too
                for g, w in zip(got, ref):
                    assert same_bits(g[s], w[s]), (s, cut)
    # a stop sequence that completes at the same step as the leaf wins; a budget equal to the leaf's step loses
    restore(m, start)
    r = m.decode_batch_constrained(first, steps, start=[0] * n, seeds=seeds, stops=[spelled[0][-2:]], max_new=[int(v) for v in ln], **KW["nucleus"])
    assert np.array_equal(r[0], ids) and np.array_equal(r[1], ln) and np.array_equal(r[4], q)
    assert [int(v) for v in r[2]] == [2 if spelled[s][-2:] == spelled[0][-2:] else eng.STOP_CONSTRAINT for s in range(n)]
    # a slot that stands on a leaf cannot start a call; greedy spells a choice too
    assert lib_rc(eng, m, first, steps) == E_ARG
    restore(m, start)
    g_ids, g_ln, g_rs, _, g_q = m.decode_batch_constrained(first[:1], steps, start=[0])
    assert g_ids[0, : g_ln[0]].tolist() in cc.CHOICES and g_rs[0] == eng.STOP_CONSTRAINT
    m.constraint_clear()


def lib_rc(eng, m, first, steps, start=None, pick=None, reserved=0, seeds=None, bias=None):
    """the status of a raw rwkv_decode_batch_constrained call (greedy by default, no stop, no record)"""
    n = len(first)
    u64, u32 = C.c_uint64, C.c_uint32
    pk = pick or eng.Pick(eng.PICK_GREEDY, 1.0, 0.8, 0, eng.nucleus_params())
    st = None if start is None else (u32 * n)(*start)
    bp = bt = bv = None
    if bias is not None:
        bp, bt, bv = (u32 * len(bias[0]))(*bias[0]), (u32 * max(1, len(bias[1])))(*bias[1]), (C.c_float * max(1, len(bias[2])))(*bias[2])
    cp = eng.ConstrainParams(st, bp, bt, bv, None, reserved)
    out, ln = (u64 * (n * steps))(), (u32 * n)()
    sd = None if seeds is None else (u64 * n)(*seeds)
    return int(eng.lib().rwkv_decode_batch_constrained(m._h, (u64 * n)(*first), n, steps, C.byref(pk), sd, C.byref(cp), None, None, out, ln, None, None))


@pytest.mark.parametrize("kind", ["greedy", "nucleus"])
def test_a_keep_continuation_gives_the_one_call(eng, model, start, kind):
    m, n, a = model, 5, cc.loop_automaton()
    first, seeds, q0 = firsts_of(n), seeds_of(n), [1, 2, 3, 4, 5]
    m.constraint_set(*a)
    restore(m, start)
    full = m.decode_batch_constrained(first, 16, start=q0, seeds=seeds, **KW[kind])
    restore(m, start)
    x = m.decode_batch_constrained(first, 8, start=q0, seeds=seeds, **KW[kind])
    y = m.decode_batch_constrained(x[0][:, 7].tolist(), 8, start=None, seeds=[s + 8 for s in seeds], keep=True, **KW[kind])
    assert np.array_equal(np.concatenate([x[0], y[0]], axis=1), full[0]) and np.array_equal(y[4], full[4])
    assert (x[1] == 8).all() and (y[1] == 8).all() and (full[1] == 16).all() and not full[2].any() and not y[2].any()
    m.constraint_clear()


# ---- rejected calls ---------------------------------------------------------------------------------------------------------------
def test_rejected_calls_leave_everything_alone(eng, model, start):
    lib, m, a = eng.lib(), model, cc.loop_automaton()
    u32 = C.c_uint32
    m.constraint_set(*a)
    restore(m, start)
    m.decode_batch_constrained(firsts_of(2), 4, start=[1, 2], seeds=seeds_of(2), **KW["nucleus"])
    probe = m.pick_constrained("greedy", row=1, slot=1, advance=False)
    state, resident, q = slots(m, MAXN, True), m.resident_bytes(), m.constraint_state_get().tolist()
    first = [5, 6]
    nuc = lambda **k: eng.Pick(eng.PICK_NUCLEUS, 1.0, 0.8, 0, eng.nucleus_params(**k))
    assert lib_rc(eng, m, first, 4, reserved=1) == E_ARG
    assert lib_rc(eng, m, first, 4, pick=eng.Pick(eng.PICK_TYPICAL, 1.0, 0.8, 0, eng.nucleus_params()), seeds=[1, 2]) == E_ARG
    assert lib_rc(eng, m, first, 4, pick=eng.Pick(7, 1.0, 0.8, 0, eng.nucleus_params())) == E_ARG
    assert lib_rc(eng, m, first, 4, start=[6, 0]) == E_ARG                                  # a start state >= S
    assert lib_rc(eng, m, first, 4, pick=nuc(), seeds=None) == E_ARG and lib_rc(eng, m, first, 4, pick=nuc(temp=0.0), seeds=[1, 2]) == E_ARG
    assert lib_rc(eng, m, [5, V], 4) == E_ARG and lib_rc(eng, m, first, 0) == E_ARG and lib_rc(eng, m, [1] * (MAXN + 1), 4) == E_ARG
    for bias in (([0, 1, 2], [0, 5], [1.0, 1.0]), ([0, 2, 2], [5, 5], [1.0, 1.0]), ([0, 2, 2], [6, 5], [1.0, 1.0]), ([0, 1, 2], [5, V], [1.0, 1.0]),
                 ([0, 1, 2], [5, 6], [1.0, np.nan]), ([0, 1, 2], [5, 6], [np.inf, 1.0]), ([1, 1, 2], [5, 6], [1.0, 1.0]), ([0, 2, 1], [5, 6], [1.0, 1.0]),
                 ([0, 301, 301], list(range(1, 302)), [0.0] * 301)):
        assert lib_rc(eng, m, first, 4, bias=bias) == E_ARG, bias
    cp = eng.ConstrainParams(None, (u32 * 3)(0, 1, 2), None, None, None, 0)                 # bias_ptr without bias_tok / bias_val
    pk = eng.Pick(eng.PICK_GREEDY, 1.0, 0.8, 0, eng.nucleus_params())
    out, ln = (C.c_uint64 * 8)(), (u32 * 2)()
    call = lambda cp_, ln_=ln: int(lib.rwkv_decode_batch_constrained(m._h, (C.c_uint64 * 2)(5, 6), 2, 4, C.byref(pk), None, cp_, None, None, out, ln_, None, None))
    assert call(C.byref(cp)) == E_ARG and call(None) == E_ARG
    assert call(C.byref(eng.ConstrainParams(None, None, None, None, None, 0)), None) == E_ARG      # out_len is required
    # malformed automata: the previous one stays installed
    for rule, kw in cc.malformed():
        if "S" not in kw:
            continue
        au = eng.Automaton(kw["S"], 0, len(kw["tok"]), kw["row_ptr"].ctypes.data_as(C.POINTER(u32)), kw["tok"].ctypes.data_as(C.POINTER(u32)),
                           kw["next"].ctypes.data_as(C.POINTER(u32)))
        assert lib.rwkv_constraint_set(m._h, C.byref(au)) == E_ARG and rule in lib.rwkv_last_error().decode(), rule
    with pytest.raises(eng.RWKVError):
        m.constraint_state_set([6])
    with pytest.raises(eng.RWKVError):
        m.constraint_state_set([0], slot0=MAXN)
    with pytest.raises(eng.RWKVError):
        m.pick_constrained("typical", row=0, slot=0)
    with pytest.raises(eng.RWKVError):
        m.pick_constrained("greedy", row=MAXN, slot=0)
    with pytest.raises(eng.RWKVError):
        m.pick_constrained("greedy", bias={0: 1.0})
    for x, y in zip(state, slots(m, MAXN, True)):
        assert same_bits(x, y)
    assert m.resident_bytes() == resident and m.constraint_state_get().tolist() == q
    assert m.pick_constrained("greedy", row=1, slot=1, advance=False) == probe             # the installed automaton is the one it was
    # not loaded; a pipeline stage; a context without the chunk path runs one stream only
    e = eng.RWKV(resident=True)
    assert lib_rc(eng, e, first, 4) == E_STATE
    e.close()
    e = load(eng, L, 48, 42, 3)
    assert lib_rc(eng, e, first, 4) == E_STATE and lib_rc(eng, e, [5], 4) == 0
    e.close()
    m.constraint_clear()
    assert lib_rc(eng, m, first, 4, start=[1, 0]) == E_ARG                                  # without an automaton only state 0


# ---- accounting -------------------------------------------------------------------------------------------------------------------
def test_the_buffers_are_counted_and_a_plain_until_call_allocates_nothing_new(eng):
    D, n, maxn = 64, 4, 8
    m = load(eng, L, D, 9, maxn)
    a = cc.loop_automaton()
    S, nnz = len(a[0]) - 1, len(a[1])
    r0 = m.resident_bytes()
    m.constraint_set(*a)
    assert m.resident_bytes() - r0 == 4 * (S + 1 + 2 * nnz) + 4 * S * cc.WORDS + 4 * maxn   # the CSR, the mask, q
    r1 = m.resident_bytes()
    m.decode_batch_constrained(firsts_of(n), 8, start=[0] * n, max_new=[8] * n)
    r2 = m.resident_bytes()
    assert r2 - r1 >= 4 * maxn * V                                                          # the second row buffer (and the call's buffers)
    m.decode_batch_until(firsts_of(n), 8, max_new=[8] * n)
    m.decode_batch_constrained(firsts_of(n - 1), 6, start=[0] * (n - 1))
    assert m.resident_bytes() == r2                                                         # a plain until call after it allocates nothing new
    m.constraint_clear()
    assert m.resident_bytes() == r2 - 4 * (S + 1 + 2 * nnz) - 4 * S * cc.WORDS              # the CSR and the mask go with the automaton
    m.close()


# ---- bindings -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_file(tmp_path_factory):
    return support.model_file(tmp_path_factory, "constrain", L, D_LOOP, 43, head_scale=30.0)


def test_constrain_app_matches_the_python_engine(eng, built, model_file, tmp_path):
    n, steps = 3, 6
    rc, lines, raw = run_app(build_app("constrain_app", tmp_path), [model_file, n, steps])
    assert rc == 0, raw
    lines = [l.split() for l in lines]
    assert lines[-1] == ["constrain_ok"] and len(lines) == 2 * n + 2
    m = eng.RWKV(resident=True)
    m.loadFile(model_file, n)
    m.forward([5, 6, 7], eng.MODE_GPT)
    for s in range(1, n):
        m.copy_state(s, 0)
    m.constraint_set(*eng.constraint_trie(cc.CHOICES))
    first, seeds = [100 + s for s in range(n)], list(range(n))
    runs = dict(greedy=m.decode_batch_constrained(first, steps, start=[0] * n),
                nucleus=m.decode_batch_constrained(first, steps, start=[0] * n, seeds=seeds, bias=[{100: -np.inf}, {}, {}], **KW["nucleus"]))
    m.forward(first[0])
    m.constraint_state_set([0])
    pick = m.pick_constrained("greedy")
    m.close()
    for f in lines[: 2 * n]:
        ids, ln, rs, _, q = runs[f[0]]
        s = int(f[1])
        assert [int(v) for v in f[2:5]] == [ln[s], rs[s], q[s]] and [int(v) for v in f[5:]] == ids[s].tolist(), f
    assert runs["nucleus"][0][0, :4].tolist() == cc.CHOICES[3]                               # the banned first token leaves one answer
    assert lines[-2] == ["pick", str(pick[0]), str(pick[1])]


def test_pybind_decode_constrained_matches_the_python_engine(eng, rwkv_mod, model_file):
    rwkv = rwkv_mod
    a = eng.constraint_trie(cc.CHOICES)
    h = rwkv.initRwkv()
    rwkv.loadModel(h, model_file)
    rwkv.initOutput(h); rwkv.initState(h)
    rwkv.setConstraint(h, *a)
    got = [rwkv.decodeConstrained(h, 1234, 8, greedy=True), rwkv.decodeConstrained(h, 1234, 8, seed=5, bias_tok=[100], bias_val=[-np.inf], **NUC)]
    rwkv.clearConstraint(h)
    rwkv.freeRwkv(h)
    m = eng.RWKV(resident=True)
    m.loadFile(model_file)                           # maxGPT 1, as loadModel
    m.constraint_set(*a)
    want = [m.decode_batch_constrained([1234], 8, start=[0])]
    want.append(m.decode_batch_constrained([1234], 8, start=[0], seeds=[5], bias=[{100: -np.inf}], **KW["nucleus"]))
    m.close()
    for (ids, reason, q), w in zip(got, want):
        assert ids == w[0][0, : w[1][0]].tolist() and reason == w[2][0] == eng.STOP_CONSTRAINT and q == w[4][0]
    assert got[1][0] == cc.CHOICES[3]
