"""Speculative sampling with a draft model that samples (include/rwkv_mi355x.h rwkv_spec_ratio_rows / rwkv_spec_verify_ratio /
rwkv_decode_speculative_sampled, csrc/ratio.hip.h).  The pick is held, pick by pick and flag by flag, to the f64 numpy restatement of the rule in
tests/ratio_cases.py on planted row pairs; no draw is excused (the case builder has asserted that each is decided with room).  The verify is
held to that rule on its own downloaded rows and, bit for bit, to rwkv_forward of the accepted rows; the loop to a host loop of public pieces."""
import ctypes as C

import numpy as np
import pytest

import ratio_cases as rc
from sampler_cases import splitmix_u
from support import E_ARG, E_STATE, GuardContexts, check_refused, eng, load, plant_rows, restore, rows, same_state, snapshot  # noqa: F401

pytestmark = pytest.mark.gpu
V, L, D, MAXT = rc.V, 2, 64, 34
DRAWS = rc.draws()


@pytest.fixture(scope="module")
def pair(eng):
    """the target and a second small context whose logits buffer holds the draft's rows"""
    t, d = load(eng, L, D, 4200, MAXT), load(eng, L, D, 4201, MAXT)
    t.forward([5, 6, 7], eng.MODE_GPT)
    d.forward([5, 6, 7], eng.MODE_GPT)
    yield t, d
    t.close(), d.close()


@pytest.mark.parametrize("n", [1, 3, 32])
@pytest.mark.parametrize("name", list(DRAWS))
def test_picks_equal_the_f64_rule(eng, pair, name, n):
    t, d = pair
    ds = DRAWS[name]
    for first in range(0, len(ds) if n == 1 else 1):                       # one row per call: every draw of the case in turn
        call = [ds[(first + i) % len(ds)] for i in range(n)]
        for group in {(c[3], c[4]) for c in call}:                         # one pair of temperatures per call
            part = [c for c in call if (c[3], c[4]) == group]
            plant_rows(t, {i + 1: c[0] for i, c in enumerate(part)}, MAXT)      # (row i + 1: the rows of a call need not start at 0)
            plant_rows(d, {i: c[1] for i, c in enumerate(part) if c[1] is not None}, MAXT)
            q = d if any(c[1] is not None for c in part) else None
            got = t.spec_ratio_rows([i + 1 for i in range(len(part))], q, [c[2] for c in part], [c[5] for c in part], [c[6] for c in part], *group)
            want = [rc.Rule(*c[:5]).pick(c[5], c[6]) for c in part]
            assert list(zip(*got)) == want, (name, n, first)
            assert all(tok != c[2] for (tok, acc), c in zip(want, part) if not acc) and all(tok != 0 for tok, _ in want)


def test_verify_ratio_commits_the_accepted_rows_exactly(eng, pair):
    t, d = pair
    start = snapshot(t, MAXT)
    token, draft, seed = 4242, [17, 40000, 911, 50276, 3], 77
    t.forward([token] + draft, eng.MODE_GPT)
    p_rows = t.logits(len(draft) + 1).reshape(-1, V).copy()
    for reject, step0 in ((None, 0), (3, 10), (1, 5)):                     # all of the draft stands; the first rejection at row 3, at row 1
        q_rows = p_rows[: len(draft)].copy()                               # q bitwise p: accepted, except where q is raised on the draft id
        tail = list(draft)
        if reject is not None:
            q_rows[reject, draft[reject]] += 30.0
            tail[reject + 1:] = [9, 8, 7][: len(draft) - reject - 1]       # the ids behind the rejection do not matter
        for ids in (draft, tail):
            plant_rows(d, {j: q_rows[j] for j in range(len(draft))}, MAXT)
            restore(t, start)
            a, nx = t.spec_verify_ratio(token, ids, d, seed, step0, 0.9, 0.9)
            a_want, nx_want, decided = rc.verify_ref(t.logits(len(draft) + 1).reshape(-1, V), q_rows, ids, 0.9, 0.9, seed, step0)
            assert decided and (a, nx) == (a_want, nx_want) and a == (len(draft) if reject is None else reject)
            got, got_rows = snapshot(t, MAXT), rows(t, a + 1)
            restore(t, start)
            t.forward([token] + draft[:a], eng.MODE_GPT)
            same_state(got, snapshot(t, MAXT), f"reject {reject}")
            assert np.array_equal(got_rows, rows(t, a + 1))
    restore(t, start)


def host_loop(eng, t, d, first, n, k, Tt, Td, seed, draft_seed):
    """rwkv_decode_speculative_sampled composed from the public pieces: the draft's sampled steps, rwkv_forward, rwkv_spec_ratio_rows"""
    out, token, drawn, stats = [], first, 0, dict(rounds=0, drafted=0, accepted=0)
    q_addr = int(eng.lib().rwkv_logits_device(d._h)) + 4 * V               # the draft's rows 1 .. k hold the stash
    while len(out) < n:
        kd = min(k, n - len(out) - 1)
        snaps, x, q_rows, feed = [], [], {}, token
        for i in range(kd + 1):
            d.forward([feed], eng.MODE_GPT)
            snaps.append(snapshot(d, 1))
            if i < kd:
                q_rows[i + 1] = d.logits(1).copy()
                feed = d.sample_nucleus(Td, 1.0, u=splitmix_u(draft_seed, drawn), ban0=True)
                x, drawn = x + [feed], drawn + 1
        plant_rows(d, q_rows, MAXT)
        start = snapshot(t, 1)
        if kd:
            t.forward([token] + x, eng.MODE_GPT)
        else:
            t.spec_verify(token, [])                                       # one row: the chunk path's one-row pass
        s = len(out)
        picks, acc = t.spec_ratio_rows(list(range(kd + 1)), q_addr if kd else None, x + [None], [splitmix_u(seed, 2 * (s + j)) for j in range(kd + 1)],
                                       [splitmix_u(seed, 2 * (s + j) + 1) for j in range(kd + 1)], Tt, Td)
        a = acc.index(0)
        if kd:
            restore(t, start)
            t.forward([token] + x[:a], eng.MODE_GPT) if a else t.spec_verify(token, [])
        restore(d, snaps[a])
        out, token = out + x[:a] + [picks[a]], picks[a]
        stats = dict(rounds=stats["rounds"] + 1, drafted=stats["drafted"] + kd, accepted=stats["accepted"] + a)
    return out, stats


def test_sampled_loop_equals_the_host_loop_and_chains(eng):
    # the draft is the target's own weights, run by the decode kernels: at another temperature some of its ids stand and some do not
    t, d = load(eng, L, D, 4200, MAXT), load(eng, L, D, 4200, MAXT)
    for m in (t, d):
        m.forward([5, 6, 7], eng.MODE_GPT)
    st, sd = snapshot(t, 1), snapshot(d, 1)
    want, wstats = host_loop(eng, t, d, 11, 14, 3, 0.8, 1.6, 31, 57)
    restore(t, st), restore(d, sd)
    got, stats = t.decode_speculative_sampled(d, 11, 14, 3, 0.8, 1.6, 31, 57)
    assert list(got) == want and stats == wstats
    assert stats["rounds"] + stats["accepted"] == 14 and 0 < stats["accepted"] < stats["drafted"] and 0 not in got
    # chaining: at equal temperatures that draft stands entirely (the decode kernels and the chunk path agree to ~1e-6), so no round of the
    # first call is cut short, and two chained calls give the ids of one
    restore(t, st), restore(d, sd)
    one, _ = t.decode_speculative_sampled(d, 11, 14, 3, 0.8, 0.8, 31, 57)
    restore(t, st), restore(d, sd)
    a, sa = t.decode_speculative_sampled(d, 11, 8, 3, 0.8, 0.8, 31, 57)
    assert sa == dict(rounds=2, drafted=6, accepted=6), sa                 # the precondition of exact chaining
    b, sb = t.decode_speculative_sampled(d, int(a[-1]), 6, 3, 0.8, 0.8, 31 + 2 * 8, 57 + sa["drafted"])
    assert list(a) + list(b) == list(one)
    t.close(), d.close()


def _refused():
    u64, dbl, one = C.c_uint64 * 2, C.c_double * 2, (C.c_uint64 * 2)(1, 1)
    rows_call = lambda n=2, q=8, draft=(5, 6), p=(1.0, 1.0, 0, 0), ua=(0.5, 0.5), ur=(0.5, 0.5): (
        lambda h, eng: (h["M"], one, C.c_void_p(q), u64(*draft), n, C.byref(eng.RatioParams(*p)), dbl(*ua), dbl(*ur), u64(), None))
    return [
        ("rwkv_spec_ratio_rows", rows_call(p=(0.0, 1.0, 0, 0)), "temp_target > 0"),
        ("rwkv_spec_ratio_rows", rows_call(p=(1.0, float("nan"), 0, 0)), "temp_draft > 0"),
        ("rwkv_spec_ratio_rows", rows_call(p=(1.0, 1.0, 1, 0)), "flag"),
        ("rwkv_spec_ratio_rows", rows_call(p=(1.0, 1.0, 0, 2)), "reserved"),
        ("rwkv_spec_ratio_rows", rows_call(ua=(0.5, 1.0)), "0 <= u < 1"),
        ("rwkv_spec_ratio_rows", rows_call(ur=(-0.1, 0.5)), "0 <= u < 1"),
        ("rwkv_spec_ratio_rows", rows_call(q=None), "q_logits is NULL"),
        ("rwkv_spec_ratio_rows", rows_call(draft=(5, V)), "draft id"),
        ("rwkv_spec_ratio_rows", rows_call(n=33), "1..32"),
        ("rwkv_spec_verify_ratio", lambda h, eng: (h["M"], 5, u64(6, 7), 2, None, C.byref(eng.RatioParams(1, 1, 0, 0)), 1, 0, u64(), u64()), "q_logits is NULL"),
        ("rwkv_spec_verify_ratio", lambda h, eng: (h["M"], 5, u64(6, 7), 2, C.c_void_p(8), C.byref(eng.RatioParams(-1, 1, 0, 0)), 1, 0, u64(), u64()), "temp_target > 0"),
        ("rwkv_decode_speculative_sampled", lambda h, eng: (h["M"], h["M"], 5, 4, 2, C.byref(eng.RatioParams(1, 1, 0, 0)), 1, 2, u64(), None), "another context"),
        ("rwkv_decode_speculative_sampled", lambda h, eng: (h["M"], h["U"], 5, 4, 2, C.byref(eng.RatioParams(1, 1, 0, 0)), 1, 2, u64(), None), "not loaded"),
    ]


def test_refused_calls_launch_nothing(eng):
    ctx = GuardContexts(eng, L, D, 8)
    for entry, args, text in _refused():
        check_refused(ctx, entry, args(ctx.h, eng), E_STATE if text == "not loaded" else E_ARG, text)
    ctx.close()
