"""DRY and no-repeat-n-gram penalties on the device (csrc/dry.hip.h k_dry_scan; rwkv_dry_history_set / _get, rwkv_debug_dry_scan,
rwkv_decode_batch_dry).  The scan alone on the planted histories of tests/dry_cases.py: the (id, L) sets exactly those of the Python restatement.
The loops bit for bit against the caller's loop they replace (forward, download the row, the numpy constrained row, the restatement's penalty on
it, the existing host pick): ids, lengths, reasons, the histories and the constrained row.  Every context is a synthetic 2-layer model.  No
tolerance anywhere: the penalty is one f32 subtraction on numbers both sides hold."""
import ctypes as C

import numpy as np
import pytest

import constraint_cases as cc
import dry_cases as dc
import sampler_cases
from support import E_ARG, V, eng, firsts_of, load, plant_rows, restore, same_bits, seeds_of, slots, start_state  # noqa: F401

pytestmark = pytest.mark.gpu

L, D, MAXN, STEPS = 2, 256, 4, 24
NUC = dict(temp=1.0, top_p=0.9, presence=0.4, frequency=0.4, decay=0.996)
KW = dict(greedy=dict(pick="greedy"), nucleus=dict(pick="nucleus", **NUC))
BAN = dict(multiplier=np.inf, base=1.0, allowed_length=2)                 # no trigram twice: three ids at +50 must run into it within 11 steps
SOFT = dict(multiplier=0.8, base=1.75, allowed_length=2)
EVERY = np.arange(V) > 0                                                  # the implicit state of a call without an automaton


@pytest.fixture(scope="module")
def model(eng):
    m = load(eng, L, D, 61, MAXN)                      # (the plain head: logits far inside the +50 of the bias lists)
    yield m
    m.close()


@pytest.fixture(scope="module")
def start(eng, model):
    return start_state(eng, model, MAXN)


def streams(n):
    """per stream: three ids to bias by +50, the history to plant -- of different lengths, the last one past the ring's wrap, each ending so
    that the first token completes a trigram the history holds -- and that first token"""
    rng = np.random.default_rng(17)
    bias = [{1000 + 10 * s: 50.0, 2000 + 10 * s: 50.0, 3000 + 10 * s: 50.0} for s in range(n)]
    hist = [[int(t) for t in rng.integers(40000, V, (5, 700, 4100, 2000)[s])] + list(b) + list(b)[:2] for s, b in enumerate(bias)]
    return bias, hist, [list(b)[2] for b in bias]


def plant(m, hist):
    for s, h in enumerate(hist):
        m.dry_history_set(h, s)


def callers_loop(eng, m, first, seeds, kind, steps, dry, bias, hist0):
    """what a caller does today, per step: forward; download the rows; the numpy constrained row; the restatement's penalty; plant it;
    sample_nucleus (or numpy argmax).  Returns ids [n][steps], the histories, the penalised rows of step 0 and the number of picks that the
    penalty changed"""
    n = len(first)
    ids, hist, fed, changed, row0 = np.zeros((n, steps), np.int64), [list(h) for h in hist0], list(first), 0, None
    for s in range(n):
        m.penalty_set(s, None)
    for k in range(steps):
        m.forward(int(fed[0])) if n == 1 else m.forward([int(t) for t in fed], eng.MODE_PARRALEL)
        rows = m.logits(n).reshape(n, V).copy()
        for s in range(n):
            hist[s].append(int(fed[s]))
        plain = [cc.constrained(rows[s], EVERY, bias[s]) for s in range(n)]
        c = [dc.penalised(plain[s], hist[s], **dry) for s in range(n)]
        row0 = c if k == 0 else row0
        for s in range(n):
            if kind == "greedy":
                ids[s, k], free = cc.argmax_low(c[s]), cc.argmax_low(plain[s])
            else:
                u = sampler_cases.splitmix_u(seeds[s], k)
                plant_rows(m, {s: plain[s]}, MAXN)
                free = m.sample_nucleus(u=u, row=s, slot=s, ban0=False, update=False, **NUC)
                plant_rows(m, {s: c[s]}, MAXN)
                ids[s, k] = m.sample_nucleus(u=u, row=s, slot=s, ban0=False, update=True, **NUC)
            changed += int(free != ids[s, k])
        plant_rows(m, {s: rows[s] for s in range(n)}, MAXN)
        fed = ids[:, k].tolist()
    return ids, hist, row0, changed


# ---- the scan alone -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(dc.CASES))
def test_scan_on_planted_histories(model, name):
    hist, kw = dc.CASES[name]
    model.dry_history_set(hist, 1)
    ids, total = model.dry_history_get(1)
    assert ids.tolist() == hist[-dc.MAX_WINDOW:] and total == len(hist)
    assert model.debug_dry_scan(1, **kw) == dc.expected(name)


def test_four_slots_hold_histories_of_different_lengths(model):
    names = ["ring_wraps_4097", "two_ids", "one_bucket", "match_65"]
    for s, nm in enumerate(names):
        model.dry_history_set(dc.CASES[nm][0], s)
    for s, nm in enumerate(names):
        assert model.debug_dry_scan(s, **dc.CASES[nm][1]) == dc.expected(nm), nm
    model.dry_history_set([], 2)
    assert model.dry_history_get(2)[1] == 0 and model.debug_dry_scan(2, allowed_length=1) == [] and model.dry_history_get(3)[1] == len(dc.CASES["match_65"][0])


# ---- the loops against the caller's loop they replace ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dry", [BAN, SOFT], ids=["ban", "soft"])
@pytest.mark.parametrize("kind", ["greedy", "nucleus"])
@pytest.mark.parametrize("n", [1, 3, 4])
def test_the_loop_is_the_callers_loop_it_replaces(eng, model, start, n, kind, dry):
    m = model
    bias, hist0, first = streams(n)
    seeds = seeds_of(n)
    restore(m, start)
    w_ids, w_hist, w_row0, changed = callers_loop(eng, m, first, seeds, kind, STEPS, dry, bias, hist0)
    restore(m, start); plant(m, hist0)
    ids, ln, rs, ran, _ = m.decode_batch_dry(first, STEPS, bias=bias, seeds=seeds, **dry, **KW[kind])
    assert changed >= 1 or dry is SOFT                                                   # a condition on the inputs: the ban must have fired
    assert np.array_equal(ids, w_ids) and ln.tolist() == [STEPS] * n and rs.tolist() == [0] * n and ran == STEPS
    for s in range(n):
        got, total = m.dry_history_get(s)
        assert got.tolist() == w_hist[s][-dc.MAX_WINDOW:] and total == len(w_hist[s]) == len(hist0[s]) + STEPS
    restore(m, start); plant(m, hist0)
    one = m.decode_batch_dry(first, 1, bias=bias, seeds=seeds, **dry, **KW[kind])
    assert np.array_equal(one[0][:, 0], w_ids[:, 0])
    for s in range(n):
        assert same_bits(m.debug_constrained_row(s), w_row0[s]), s
        assert dry is SOFT or w_row0[s][min(bias[s])] == -np.inf                          # the planted trigram was banned at step 0


def test_a_stop_sequence_ends_a_stream_and_its_history(eng, model, start):
    m, n = model, 3
    bias, hist0, first = streams(n)
    restore(m, start); plant(m, hist0)
    full = m.decode_batch_dry(first, STEPS, bias=bias, **BAN)
    stop = full[0][1][4:6].tolist()
    cut = next(k + 1 for k in range(1, STEPS) if full[0][1][k - 1: k + 1].tolist() == stop)
    restore(m, start); plant(m, hist0)
    ids, ln, rs, ran, _ = m.decode_batch_dry(first, STEPS, bias=bias, stops=[stop], **BAN)
    got = slots(m, n, False)
    assert ln.tolist() == [STEPS, cut, STEPS] and rs.tolist() == [0, 2, 0] and cut <= 6
    assert np.array_equal(ids[[0, 2]], full[0][[0, 2]]) and np.array_equal(ids[1, :cut], full[0][1, :cut]) and not ids[1, cut:].any()
    h, total = m.dry_history_get(1)
    assert h.tolist() == (hist0[1] + [first[1]] + ids[1, : cut - 1].tolist())[-dc.MAX_WINDOW:] and total == len(hist0[1]) + cut
    restore(m, start); plant(m, hist0)
    m.decode_batch_dry(first, cut, bias=bias, **BAN)
    for g, w in zip(got, slots(m, n, False)):
        assert same_bits(g[1], w[1])                                                      # the slot is what the shorter call leaves


@pytest.mark.parametrize("kind", ["greedy", "nucleus"])
def test_a_keep_continuation_gives_the_one_call(eng, model, start, kind):
    m, n = model, 3
    bias, hist0, first = streams(n)
    seeds = seeds_of(n)
    restore(m, start); plant(m, hist0)
    full = m.decode_batch_dry(first, 16, bias=bias, seeds=seeds, **SOFT, **KW[kind])
    want = [m.dry_history_get(s) for s in range(n)]
    restore(m, start); plant(m, hist0)
    x = m.decode_batch_dry(first, 8, bias=bias, seeds=seeds, **SOFT, **KW[kind])
    y = m.decode_batch_dry(x[0][:, 7].tolist(), 8, bias=bias, seeds=[s + 8 for s in seeds], keep=True, **SOFT, **KW[kind])
    assert np.array_equal(np.concatenate([x[0], y[0]], axis=1), full[0])
    for s in range(n):
        got = m.dry_history_get(s)
        assert got[0].tolist() == want[s][0].tolist() and got[1] == want[s][1]


@pytest.mark.parametrize("kind", ["greedy", "nucleus"])
@pytest.mark.parametrize("n", [1, 3])
def test_multiplier_zero_is_the_constrained_call(eng, model, start, n, kind):
    m = model
    bias, hist0, first = streams(n)
    plant(m, hist0)
    restore(m, start)
    want = m.decode_batch_constrained(first, 6, bias=bias, seeds=seeds_of(n), **KW[kind])
    w_rows = [m.debug_constrained_row(s) for s in range(n)]
    restore(m, start)
    got = m.decode_batch_dry(first, 6, bias=bias, seeds=seeds_of(n), multiplier=0.0, **KW[kind])
    assert np.array_equal(got[0], want[0]) and all(same_bits(m.debug_constrained_row(s), w_rows[s]) for s in range(n))
    assert [m.dry_history_get(s)[1] for s in range(n)] == [len(h) for h in hist0]         # off: nothing is appended


# ---- rejected calls -------------------------------------------------------------------------------------------------------------------
BAD = [dict(multiplier=-0.5), dict(multiplier=np.nan), dict(base=0.99), dict(base=np.inf), dict(base=np.nan), dict(allowed_length=0), dict(allowed_length=65),
       dict(window=0), dict(window=4097), dict(n_breakers=33), dict(n_breakers=1, breakers=None), dict(n_breakers=1, breakers=[V]), dict(flags=1),
       dict(reserved=1), dict(kind=1), dict(first=V), dict(steps=0), dict(hist=[V])]


@pytest.fixture(scope="module")
def bare(eng):
    """a context on which no generation call has run and no history was set: whatever a call allocates shows in resident_bytes"""
    m = load(eng, L, 64, 62, 1)
    resident = m.resident_bytes()
    yield m
    assert m.resident_bytes() == resident                                                 # none of the rejected calls allocated
    m.decode_batch_dry([5], 2)
    assert m.resident_bytes() > resident and m.dry_history_get(0)[1] == 2                 # an accepted one does, and appends
    m.close()


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_rejected_calls_launch_and_allocate_nothing(eng, bare, bad):
    m, lib = bare, eng.lib()
    f = dict(multiplier=0.8, base=1.75, allowed_length=2, window=4096, n_breakers=0, breakers=None, flags=0, reserved=0, kind=0, first=5, steps=4, hist=None)
    f.update(bad)
    br = None if f["breakers"] is None else (C.c_uint32 * len(f["breakers"]))(*f["breakers"])
    p = eng.DryParams(f["multiplier"], f["base"], f["allowed_length"], f["window"], f["n_breakers"], f["flags"], br, f["reserved"])
    pk = eng.Pick(f["kind"], 1.0, 0.8, 0, eng.nucleus_params())
    out, ln, tok, cnt = (C.c_uint64 * 8)(), (C.c_uint32 * 1)(), (C.c_uint32 * 4096)(), C.c_uint32(0)
    resident = m.resident_bytes()
    if f["hist"] is not None:
        assert lib.rwkv_dry_history_set(m._h, 0, (C.c_uint64 * 1)(*f["hist"]), 1) == E_ARG
    else:
        assert lib.rwkv_decode_batch_dry(m._h, (C.c_uint64 * 1)(f["first"]), 1, f["steps"], C.byref(pk), (C.c_uint64 * 1)(1), None, C.byref(p), None, None,
                                         out, ln, None, None) == E_ARG
        if not ({"kind", "first", "steps"} & set(bad)):
            assert lib.rwkv_debug_dry_scan(m._h, 0, C.byref(p), tok, tok, C.byref(cnt)) == E_ARG
    assert m.resident_bytes() == resident and m.dry_history_get(0)[1] == 0
