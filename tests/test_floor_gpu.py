"""The device's floor samplers (csrc/floor.hip.h) and their entry points against the f64 reference of tests/floor_cases.py: planted rows draw by
draw, the loops against the reference loop over downloaded logits, rwkv_sample_rows, refused calls.  mu stays within 1e-8 of the reference's over
64 steps: an f64 sum of 50277 terms is off by V 2^-53 ~ 6e-12, so ~2e-11 in S, times eta <= 1 over 64 steps: under 2e-9, a factor of 5 below."""
import ctypes as C

import numpy as np
import pytest

import floor_cases as fc
from support import E_ARG, GuardContexts, check_refused, eng, load, plant_rows, slots  # noqa: F401

pytestmark = pytest.mark.gpu

ROWS, V, MU_TOL, L, D, N_GEN = 4, fc.V, 1e-8, 2, 256, 16
PEN = dict(presence=0.4, frequency=0.4, decay=0.996)
LOOPS = {"minp": dict(pick="minp", temp=1.0, min_p=0.05, **PEN), "mirostat": dict(pick="mirostat", temp=0.7, tau=3.0, eta=0.5, **PEN)}
FIRST, SEEDS = [9, 4242, 30000], [11, 22, 33]


def context(*shape, **kw):
    @pytest.fixture(scope="module")
    def fixture(eng):
        m = load(eng, *shape, **kw)
        m.forward(5)
        yield m
        m.close()
    return fixture


ctx, model = context(2, 64, 3, ROWS), context(L, D, 12, ROWS, head_scale=30.0)      # for planted rows; for the loops


@pytest.mark.parametrize("label,lname,run,counted,shift,row,slot", fc.RUNS, ids=fc.IDS)
def test_planted_run_matches_the_reference(ctx, label, lname, run, counted, shift, row, slot):
    m, bad, synced = ctx, [], False
    plant_rows(m, {row: fc.logits_of(lname, run.ban0)}, ROWS)
    m.penalty_set(slot, fc.counts_of(lname, shift) if counted else None)
    for (u, ref, want, mu0, mu1, _) in fc.draws_of(lname, run, counted, shift):
        if mu0 is not None and not synced:           # in front of the first draw, and behind an excused draw that went the other way
            m.mirostat_set([mu0], slot)
            synced = True
        got = m.sample_floor(run.kind, u, row, slot, run.ban0, update=mu0 is not None, **run.kw())
        if got != want:
            synced = False
            if not (ref.excused(u) and got < V):
                bad.append((u, got, want))
        elif mu1 is not None and not abs(float(m.mirostat_get(slot)[0]) - mu1) <= MU_TOL:      # the device's own mu, carried from draw to draw
            bad.append((u, "mu", float(m.mirostat_get(slot)[0]), mu1))
    assert not bad, f"{len(bad)} draws, first (u, device, reference): {bad[:4]}"


def host_loop(eng, m, kw, n, steps, got, rows_of=None):      # the reference loop over downloaded logits (rows_of: over the constrained rows made of them)
    run = fc.Run(kw["pick"], kw["temp"], kw.get("min_p", kw.get("tau")), kw.get("eta", 0.0), ban0=True, presence=kw["presence"], frequency=kw["frequency"])
    ids, cs, mus = FIRST[:n], [np.zeros(V, np.float32) for _ in range(n)], [2.0 * kw.get("tau", 0.0)] * n
    dev_c, dev_mu = [m.penalty_get(s) for s in range(n)], m.mirostat_get(0, n).copy()
    m.reset_state()
    for k in range(steps):
        lg = (m.forward(ids[0]) if n == 1 else m.forward(ids, eng.MODE_PARRALEL))[: n * V].reshape(n, V).copy()      # (one stream runs the decode kernels)
        for s in range(n):
            r, S = fc.reference(lg[s] if rows_of is None else rows_of(lg[s]), run, cs[s], mus[s], ban0=rows_of is None)
            g, u = int(got[s][k]), fc.splitmix_u(SEEDS[s], k)
            assert g == r.pick(u) or (r.excused(u) and 0 < g < V), f"stream {s} step {k}: device {g} reference {r.pick(u)}"
            cs[s], ids[s] = fc.nc.count_update(cs[s], g, kw["decay"]), g
            mus[s] = fc.mu_next(run, S, g, mus[s]) if S is not None else dev_mu[s]
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(dev_c, cs)) and np.abs(dev_mu - np.array(mus)).max() <= MU_TOL


def until(m, n, steps, first=None, kind="mirostat", **kw):          # one call of a loop: (ids, len, reason, [state, logits, counts per slot], mu)
    if first is None:
        m.reset_state()
    ids, ln, rs, _ = m.decode_batch_until(first or FIRST[:n], steps, **{**dict(seeds=SEEDS[:n]), **LOOPS[kind], **kw})
    return ids, ln, rs, slots(m, n, True), m.mirostat_get(0, n).copy()


@pytest.mark.parametrize("kind", list(LOOPS))
@pytest.mark.parametrize("n", [1, 2, 3])
def test_decode_batch_until_equals_the_reference_loop(eng, model, kind, n):
    ids, ln, *_ = until(model, n, N_GEN, kind=kind)
    assert (ln == N_GEN).all()
    host_loop(eng, model, LOOPS[kind], n, N_GEN, ids)


@pytest.mark.parametrize("n", [1, 3])
def test_keep_splits_a_call_and_a_stop_parks_mu(model, n):
    whole, _, _, s16, mu16 = until(model, n, 16)
    a = until(model, n, 8)[0]
    b, _, _, s88, mu88 = until(model, n, 8, first=a[:, -1].tolist(), seeds=[s + 8 for s in SEEDS[:n]], keep=True)
    assert np.array_equal(np.concatenate([a, b], axis=1), whole) and np.array_equal(mu88, mu16) and np.array_equal(s88[-1], s16[-1])
    # stream 0 stopped by its budget at step 5 of 16 is left as the 5-step call leaves it; the others ran on
    _, _, _, s5, mu5 = until(model, n, 5)
    ids, ln, rs, got, mu = until(model, n, 16, max_new=[5] + [16] * (n - 1))
    assert ln[0] == 5 and rs[0] == 1 and np.array_equal(ids[0, :5], whole[0, :5])
    assert all(np.array_equal(g[0].view(np.uint8), w[0].view(np.uint8)) for w, g in zip(s5, got)) and mu[0] == mu5[0] and np.array_equal(mu[1:], mu16[1:])


def test_constrained_rows_carry_no_mass(eng, model):
    m, kw, allowed = model, LOOPS["mirostat"], np.arange(100, 50000, 7)
    m.constraint_set([0, len(allowed)], allowed, np.zeros(len(allowed), np.uint32))        # one state that loops on the allowed ids
    try:
        m.reset_state()
        ids = m.decode_batch_constrained(FIRST[:2], 8, seeds=SEEDS[:2], **kw)[0]
        assert np.isin(ids, allowed).all(), ids
        host_loop(eng, m, kw, 2, 8, ids, lambda row: np.where(np.isin(np.arange(V), allowed), row, -np.inf).astype(np.float32))
    finally:
        m.constraint_clear()


def test_sample_rows_mixes_the_four_kinds(eng, ctx):
    m = ctx
    plant_rows(m, {0: fc.logits_of("a"), 1: fc.logits_of("c"), 2: fc.logits_of("d50")}, ROWS)
    specs = [dict(row=0, kind="greedy"), dict(row=1, slot=0, kind="nucleus", u=0.3, update=True, temp=0.8, top_p=0.9, **PEN),
             dict(row=2, slot=1, kind="minp", u=0.6, update=True, temp=1.5, min_p=0.05, **PEN),
             dict(row=0, slot=2, kind="mirostat", seed=5, step=7, update=True, ban0=True, temp=0.7, tau=3.0, eta=0.5, **PEN),
             dict(row=1, slot=3, kind="minp", seed=9, step=2, min_p=0.5)]

    def run(picks):
        for s in range(3):
            m.penalty_set(s, fc.counts_of("a", s))
        m.mirostat_set([4.5] * ROWS)
        return picks(), [m.penalty_get(s) for s in range(3)], m.mirostat_get(0, ROWS).copy()

    def one_shot(q):          # the (seed, step) form draws the loops' uniform of that step
        q = dict(q)
        u = q.pop("u") if "u" in q else fc.splitmix_u(q.pop("seed"), q.pop("step"))
        if q["kind"] == "nucleus":
            return m.sample_nucleus(0.8, 0.9, 0, 0.4, 0.4, 0.996, u, row=q["row"], slot=q["slot"], update=True)
        return m.sample_floor(q.pop("kind"), u, q.pop("row"), q.pop("slot"), **q)
    got, c, mu = run(lambda: m.sample_rows([eng.pick_query(**q) for q in specs]))
    want, c1, mu1 = run(lambda: [int(np.argmax(fc.logits_of("a")[1:])) + 1] + [one_shot(q) for q in specs[1:]])
    assert list(got) == want and all(np.array_equal(a, b) for a, b in zip(c, c1)) and np.array_equal(mu, mu1) and mu[2] != 4.5 and (mu[[0, 1, 3]] == 4.5).all()


def test_refused_calls_leave_everything_as_it_was(eng):
    g = GuardContexts(eng, 2, 64, 8, counts=[np.array(fc.counts_of("a", s), np.float32) for s in range(8)])
    try:
        m, h = g.models["M"], g.h["M"]
        m.mirostat_set(np.arange(8.0))
        tok, out, ln, first, seeds, (sp, alive) = C.c_uint64(0), (C.c_uint64 * 8)(), (C.c_uint32 * 2)(), (C.c_uint64 * 2)(5, 6), (C.c_uint64 * 2)(1, 2), eng.stop_params()
        bad = [eng.floor_pick("minp", min_p=0.0), eng.floor_pick("minp", min_p=1.5), eng.floor_pick("mirostat", tau=0.0),
               eng.floor_pick("mirostat", eta=-1.0), eng.floor_pick("mirostat", eta=float("nan"))]
        for kind, tp, tk in (("minp", 0.9, 0), ("minp", 1.0, 40), ("mirostat", 0.9, 0), ("mirostat", 1.0, 40)):     # a floor combines with no other cut
            bad.append(eng.Pick(eng.PICK_KINDS[kind], 1.0, 0.5, 0, eng.nucleus_params(1.0, tp, tk, presence=0.4)))
        for pk in bad:
            check_refused(g, "rwkv_sample_floor", (h, 0, 0, C.byref(pk), 0.5, C.byref(tok)), E_ARG, "")
            check_refused(g, "rwkv_decode_batch_until", (h, first, 2, 4, C.byref(pk), seeds, C.byref(sp), out, ln, None, None), E_ARG, "")
        seg, na = eng.SpecSegment(0, 2, 1, 0), (C.c_uint32 * 1)()
        for kind in ("minp", "mirostat"):
            check_refused(g, "rwkv_spec_sample_segments", (h, first, C.byref(seg), 1, C.byref(eng.floor_pick(kind)), seeds, seeds, 0, na, out, None), E_ARG, "neither greedy nor nucleus")
        twice = (eng.PickQuery * 2)(eng.pick_query(0, 1, "mirostat", u=0.5, update=True), eng.pick_query(1, 1, "mirostat", u=0.5, update=True))
        check_refused(g, "rwkv_sample_rows", (h, twice, 2, out), E_ARG, "updated twice")
        assert np.array_equal(m.mirostat_get(0, 8), np.arange(8.0))
    finally:
        g.close()
