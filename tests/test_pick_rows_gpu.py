"""rwkv_sample_rows and rwkv_spec_sample_segments (csrc/pickrows.hip.h: k_pickq_stats, k_pickq_keys, k_pickq).
(1) Every planted case of tests/nucleus_cases.py, all runs x all draws as ONE call of independent queries, against the log-space f64 reference
there (a differing draw fails unless the reference alone excuses it; tests/test_nucleus_cpu.py caps those at 2 per run) and, without exception,
against rwkv_sample_nucleus of the same query.  (2) One mixed call across the batch boundary: greedy and nucleus, seeds, penalties with UPDATE.
(3) The sampled verify against its host composition.  (4) Refused calls answer their status and leave everything as it was."""
import ctypes as C

import numpy as np
import pytest

import nucleus_cases as nc
from support import E_ARG, E_STATE, GuardContexts, check_refused, eng, load, plant_rows, restore, rows, same_state, snapshot, start_state  # noqa: F401

pytestmark = pytest.mark.gpu

ROWS, V = 16, nc.V


@pytest.fixture(scope="module")
def ctx(eng):
    m = load(eng, 2, 64, 3, ROWS)
    m.forward(5)
    yield m
    m.close()


def nucleus_q(eng, run, row, slot, **kw):
    return eng.pick_query(row, slot, temp=run.temp, top_p=run.top_p, top_k=run.top_k, presence=run.presence, frequency=run.frequency, ban0=run.ban0, **kw)


@pytest.mark.parametrize("name", list(nc.CASES))
def test_planted_case_in_one_call(eng, ctx, name):
    case = nc.CASES[name]
    plant_rows(ctx, {1 + ban: nc.logits_of(case.logits, bool(ban)) for ban in (0, 1)}, ROWS)      # (the tie set of d1025 has one more id under the ban)
    if case.counted:
        ctx.penalty_set(3, nc.counts_of(case.logits))
    asked = [(run, u) for run in case.runs for u in nc.US]
    got = ctx.sample_rows([nucleus_q(eng, run, 1 + run.ban0, 3, u=u) for run, u in asked])
    bad = []
    for (run, u), g in zip(asked, got):
        ref = nc.ref_of(case.logits, run, case.counted)
        one = ctx.sample_nucleus(run.temp, run.top_p, run.top_k, run.presence, run.frequency, 1.0, u, row=1 + run.ban0, slot=3, ban0=run.ban0)
        if g != one or (g != ref.pick(u) and not ref.excused(u)):
            bad.append((run, u, g, one, ref.pick(u)))
    print(f"{name}: queries {len(asked)} excused {sum(nc.ref_of(case.logits, r, case.counted).excused(u) for r, u in asked)} bad {len(bad)}")
    assert not bad, f"{len(bad)} draws, first (run, u, sample_rows, sample_nucleus, reference): {bad[:4]}"


def greedy_rule(l):
    """decode_batch_greedy's pick: logit 0 banned, ties to the lowest id"""
    return 1 + int(np.argmax(np.asarray(l[1:], np.float64)))


@pytest.mark.parametrize("n", [63, 64, 67])
def test_mixed_call_across_the_batch_boundary(eng, ctx, n):
    assert eng.PICK_BATCH == 64
    ties = np.full(V, -3.0, np.float32); ties[[0, 1, V - 1]] = (9.0, 2.5, 2.5)
    planted = {5: nc.logits_of("a"), 9: nc.logits_of("c"), 2: ties, 3: np.full(V, -np.inf, np.float32)}
    plant_rows(ctx, planted, ROWS)
    cnt = {s: nc.counts_of("a", s) for s in (6, 7, 8, 0)}
    pen, plain = nc.Run(1, 0.9, 0, False, 0.4, 0.4), nc.Run(0.7, 0.5, 40, True)
    qs = [nucleus_q(eng, pen, 5, 6, seed=11, step=3, update=True, decay=1.0), nucleus_q(eng, pen, 5, 7, u=0.37, update=True, decay=0.996),
          eng.pick_query(2, 6, kind="greedy"), eng.pick_query(3, 1, kind="greedy")]
    while len(qs) < n:       # the rest: row 5 under many seeds, row 9, a slot that is only read, the greedy rows again
        k = len(qs)
        qs.append((nucleus_q(eng, plain, 5, 1, seed=k, step=2 ** 40 + k), nucleus_q(eng, pen, 9, 8, seed=7, step=k), eng.pick_query(2 + k % 2, 5, kind="greedy"))[k % 3])

    def fresh():
        for s, c in cnt.items():
            ctx.penalty_set(s, c)
    fresh()
    state0, rows0, before = snapshot(ctx, ROWS), rows(ctx, ROWS), [ctx.penalty_get(s) for s in range(ROWS)]
    got = ctx.sample_rows(qs)
    after = {s: ctx.penalty_get(s) for s in range(ROWS)}
    same_state(snapshot(ctx, ROWS), state0, "state")
    assert np.array_equal(rows(ctx, ROWS), rows0), "logits"
    for s, decay, g in ((6, 1.0, got[0]), (7, 0.996, got[1])):
        assert np.array_equal(after[s].view(np.uint32), nc.count_update(cnt[s], g, decay).view(np.uint32)), f"counts of slot {s}"
    assert all(np.array_equal(after[s].view(np.uint32), before[s].view(np.uint32)) for s in range(ROWS) if s not in (6, 7)), "counts of a slot that no query updates"
    fresh()
    assert got == [ctx.sample_rows([q])[0] for q in qs], "one call against the queries one by one"
    for q, g in zip(qs, got):
        if q.pick.kind == eng.PICK_GREEDY:
            assert g == greedy_rule(planted[q.row]) == 1      # (the tie at columns 1 and V - 1; the all -inf row)
        elif q.flags & eng.PICKQ_SEED and not q.pick.nucleus.flags & eng.NUCLEUS_UPDATE:      # the seed path against the host's draw through the u path
            by_u = eng.PickQuery.from_buffer_copy(q)
            by_u.flags, by_u.u = 0, nc.splitmix_u(q.seed, q.step)
            assert g == ctx.sample_rows([by_u])[0]
    fresh()
    assert got[0] == ctx.sample_rows([nucleus_q(eng, pen, 5, 6, u=nc.splitmix_u(11, 3))])[0]


def test_sampled_verify_against_its_host_composition(eng):
    m = load(eng, 2, 64, 3, ROWS)
    try:
        start = start_state(eng, m, 8)
        picks = [eng.pick_of(temp=1.0, top_p=0.9), eng.pick_of(temp=0.7, top_p=0.5, top_k=40), eng.pick_of(temp=1.5, top_p=1.0), eng.pick_of("greedy")]
        slots, seeds, step0 = [1, 4, 2, 7], [5, 6, 7, 8], [0, 9, 2 ** 33, 3]
        certain, nd = [[17], [40000], [9, 1234, 77], [50000]], [0, 3, 3, 2]
        chain, feed = [[] for _ in slots], certain
        for k in range(4):       # the first run: every stream's true continuation, one id per call
            out = m.spec_sample_segments([(s, f, 0) for s, f in zip(slots, feed)], picks, seeds, [s + k for s in step0])
            feed = [[nx] for (_, nx, _) in out]
            for c, f in zip(chain, feed):
                c += f
        good = [0, 1, 3, 0]      # accept none (no draft), some, all, none
        results = []
        for w in (1, 2):         # two different wrong tails behind the acceptance point
            draft = [[c[j] if j < a else c[j] % (V - w) + w for j in range(d)] for c, a, d in zip(chain, good, nd)]
            segs = [(s, c + d, len(d)) for s, c, d in zip(slots, certain, draft)]
            restore(m, start)
            got = m.spec_sample_segments(segs, picks, seeds, step0)
            state = snapshot(m, 8)
            restore(m, start)        # the host composition: the same rows forward, the uncertain rows sampled, acceptance here
            last = m.forward_segments([(s, ids) for s, ids, _ in segs])
            want, stand = [], []
            for i, (s, ids, d) in enumerate(segs):
                rc = last[i] - d
                qs = [eng.PickQuery(rc + j, s, picks[i], seeds[i], step0[i] + j, 0.0, eng.PICKQ_SEED, 0) for j in range(d + 1)]
                for q in qs:
                    q.pick.nucleus.flags |= eng.NUCLEUS_BAN0
                t = m.sample_rows(qs)
                a = next((j for j in range(d) if ids[len(ids) - d + j] != t[j]), d)
                want.append((a, t[a], rc + a))
                stand.append((s, ids[: len(ids) - d + a]))
            assert got == want and [a for a, _, _ in got] == good and [nx for _, nx, _ in got] == [c[a] for c, a in zip(chain, good)]
            restore(m, start)
            m.forward_segments(stand)
            same_state(state, snapshot(m, 8), "the slots against forward_segments of the rows that stand")
            restore(m, start)
            alone = m.spec_verify_segments([segs[3]])[0]
            assert alone[:2] == got[3][:2] and alone[2] == got[3][2] - (last[3] - len(segs[3][1]) + 1), "a greedy segment against spec_verify_segments"
            results.append((got, state))
        assert results[0][0] == results[1][0]
        same_state(results[0][1], results[1][1], "two wrong tails")
    finally:
        m.close()


@pytest.fixture(scope="module")
def guards(eng):
    g = GuardContexts(eng, 2, 64, ROWS, counts=[nc.counts_of("a")] * ROWS)
    yield g
    g.close()


def _q(eng, **kw):
    f = dict(row=0, slot=0, kind="nucleus", u=0.5)
    f.update(kw)
    extra = {k: f.pop(k) for k in ("flags", "reserved", "rawkind") if k in f}
    q = eng.pick_query(**f)
    q.flags, q.reserved, q.pick.kind = extra.get("flags", q.flags), extra.get("reserved", 0), extra.get("rawkind", q.pick.kind)
    return [q]


UPD = dict(presence=0.4, update=True)
REFUSED_ROWS = [      # (context, queries or None, n or None, status, text)
    ("M", None, 1, E_ARG, "NULL"), ("M", [{}], 0, E_ARG, "n must be in"), ("M", [{}], 1025, E_ARG, "n must be in"),
    ("M", [dict(row=ROWS)], None, E_ARG, "out of range"), ("M", [dict(slot=ROWS)], None, E_ARG, "out of range"),
    ("M", [dict(rawkind=1)], None, E_ARG, "neither greedy nor nucleus"), ("M", [dict(temp=0.0)], None, E_ARG, "temp"),
    ("M", [dict(decay=1.5)], None, E_ARG, "decay"), ("M", [dict(u=1.0)], None, E_ARG, "0 <= u < 1"), ("M", [dict(flags=2)], None, E_ARG, "unknown flag"),
    ("M", [dict(reserved=1)], None, E_ARG, "reserved"), ("M", [dict(slot=2, **UPD), {}, dict(slot=2, **UPD)], None, E_ARG, "updated twice"),
    ("M", [dict(slot=2, **UPD), dict(slot=2, presence=0.4)], None, E_ARG, "read by another"),
    ("U", [{}], None, E_STATE, "not loaded"), ("S", [{}], None, E_STATE, "head"),
]


@pytest.mark.parametrize("which,qs,n,status,text", REFUSED_ROWS)
def test_sample_rows_refuses(eng, guards, which, qs, n, status, text):
    arr = None if qs is None else (eng.PickQuery * len(qs))(*[_q(eng, **kw)[0] for kw in qs])
    out = (C.c_uint64 * 8)()
    check_refused(guards, "rwkv_sample_rows", (guards.h[which], arr, len(qs) if n is None else n, out), status, text)


REFUSED_VERIFY = [    # (context, segments (slot, n, n_draft), pick keywords or the NULL argument, flags, status, text)
    ("M", [(0, 2, 1)], "picks", 0, E_ARG, "NULL"), ("M", [(0, 2, 1)], "seeds", 0, E_ARG, "NULL"), ("M", [(0, 2, 1)], "step0", 0, E_ARG, "NULL"), ("M", [(0, 2, 1)], dict(rawkind=1), 0, E_ARG, "neither greedy nor nucleus"),
    ("M", [(0, 2, 1)], dict(frequency=0.5), 0, E_ARG, "penalties"), ("M", [(0, 2, 1)], dict(temp=-1.0), 0, E_ARG, "temp"),
    ("M", [(0, 2, 1)], {}, 1, E_ARG, "flags must be 0"), ("M", [(0, 2, 2)], {}, 0, E_ARG, "n_draft"), ("M", [(3, 1, 0), (3, 1, 0)], {}, 0, E_ARG, "named twice"),
    ("M", [(0, ROWS + 1, 0)], {}, 0, E_ARG, "Context too large"), ("U", [(0, 2, 1)], {}, 0, E_STATE, "not loaded"), ("S", [(0, 2, 1)], {}, 0, E_STATE, "whole-model"),
]


@pytest.mark.parametrize("which,segs,pick,flags,status,text", REFUSED_VERIFY)
def test_spec_sample_segments_refuses(eng, guards, which, segs, pick, flags, status, text):
    n = len(segs)
    arr = (eng.SpecSegment * n)(*[eng.SpecSegment(s, k, d, 0) for s, k, d in segs])
    toks = (C.c_uint64 * 32)(*([5] * 32))
    null = pick if isinstance(pick, str) else None
    pk = (eng.Pick * n)(*[_q(eng, **({} if null else pick))[0].pick] * n)
    u64, acc = (C.c_uint64 * n), (C.c_uint32 * n)()
    args = dict(picks=pk, seeds=u64(), step0=u64())
    args.update({null: None} if null else {})
    check_refused(guards, "rwkv_spec_sample_segments", (guards.h[which], toks, arr, n, args["picks"], args["seeds"], args["step0"], flags, acc, u64(), u64()), status, text)
