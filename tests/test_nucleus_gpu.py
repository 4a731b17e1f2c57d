"""The device nucleus sampler (csrc/nucleus.hip.h: k_nucleus_stats, k_nucleus_keys, k_nucleus) and its entry points.
(1) Every planted case of tests/nucleus_cases.py, draw by draw against the log-space f64 reference there: a device pick that differs from the
reference's is a failure unless the reference alone excuses the draw (tests/test_nucleus_cpu.py caps the excused draws at 2 per run).  Every
run prints its tally (draws, excused, mismatched) before anything is asserted.  (2) The count update is bit-equal to its f32 restatement, happens
only with UPDATE, and without penalties no count buffer exists.  (3, 4) decode_nucleus and decode_batch_nucleus against a host loop (forward,
the reference with numpy f32 counts), final counts bit-equal.  (5) KEEP: 16 steps = 8 + 8 with seed + 8.  (6) The pybind module's
decodeNucleus / nucleusSample (through include/rwkv.h, host-authoritative state) against the Python engine.  (7) Refused calls answer their status
and leave state, logits and counts bit-identical."""
import ctypes as C

import numpy as np
import pytest

import nucleus_cases as nc
from support import E_ARG, E_STATE, GuardContexts, check_refused, eng, load, plant_rows, rwkv_mod  # noqa: F401

from rwkv_cpp_accelerated_amd import modelfile as mf

pytestmark = pytest.mark.gpu

ROWS = 4                      # maxGPT of the planted context and of the loop model
V = nc.V


def planted_context(eng):
    m = load(eng, 2, 64, 3, ROWS)
    m.forward(5)
    return m


@pytest.fixture(scope="module")
def ctx(eng):
    m = planted_context(eng)
    yield m
    m.close()


def run_draws(m, label, ref, run, row=0, slot=0):
    """the 66 draws of one run on a planted row / slot; returns the failures, prints the tally"""
    excused = mismatched = 0
    bad = []
    for u in nc.US:
        got = m.sample_nucleus(run.temp, run.top_p, run.top_k, run.presence, run.frequency, 1.0, u, row=row, slot=slot, ban0=run.ban0)
        want, ex = ref.pick(u), ref.excused(u)
        excused += ex
        why = None
        if got >= V:
            why = "pick outside the vocabulary"
        elif not ref.w[got] > 0 and not ex:
            why = "a token outside the kept set"
        elif got != want and not ex:
            why = "differs from the reference"
        if why:
            mismatched += 1
            bad.append((label, run, u, got, want, why))
    print(f"{label:>8} temp {run.temp:<5} top_p {run.top_p:<5} top_k {run.top_k:<5} ban0 {int(run.ban0)} pen {run.presence}/{run.frequency}: "
          f"draws {len(nc.US)} excused {excused} mismatched {mismatched}")
    return bad


@pytest.mark.parametrize("name", list(nc.CASES))
def test_planted_case_matches_the_log_space_reference(ctx, name):
    case, bad = nc.CASES[name], []
    if case.counted:
        ctx.penalty_set(0, nc.counts_of(case.logits))
    planted = None
    for run in case.runs:
        if planted != run.ban0:                      # (the tie set of d1025 has one more id under the ban)
            plant_rows(ctx, {0: nc.logits_of(case.logits, run.ban0)}, ROWS)
            planted = run.ban0
        bad += run_draws(ctx, name, nc.ref_of(case.logits, run, case.counted), run)
    if case.counted:
        assert np.array_equal(ctx.penalty_get(0), nc.counts_of(case.logits)), "a draw without UPDATE changed the counts"
    assert not bad, f"{len(bad)} draws, first (case, run, u, device, reference, why): {bad[:4]}"


def test_rows_and_slots_are_addressed_independently_case_r(ctx):
    """three rows of different content, each sampled with the counts of a different slot"""
    plant_rows(ctx, {row: nc.logits_of(n, False) for (n, row, _) in nc.ROW_CASE}, ROWS)
    for (n, _, slot) in nc.ROW_CASE:
        ctx.penalty_set(slot, nc.counts_of(n, slot))
    bad = []
    for (n, row, slot) in nc.ROW_CASE:
        for run in nc.ROW_RUNS:
            bad += run_draws(ctx, f"r/{n}@{row}/{slot}", nc.ref_of(n, run, True, slot), run, row=row, slot=slot)
    assert not bad, f"{len(bad)} draws, first (case, run, u, device, reference, why): {bad[:4]}"


def test_count_update_is_the_f32_restatement(eng):
    m = planted_context(eng)                    # a context of its own: no count buffer yet
    try:
        lg = nc.logits_of("a")
        plant_rows(m, {0: lg}, ROWS)
        rb0 = m.resident_bytes()
        for u in (0.1, 0.5, 0.9):                   # both penalties 0: nothing is read, updated or allocated, UPDATE or not
            got = m.sample_nucleus(1.0, 0.9, 0, 0.0, 0.0, 0.996, u, update=True)
            r = nc.ref_of("a", nc.Run(1, 0.9))
            assert got == r.pick(u) or r.excused(u)
        assert m.resident_bytes() == rb0 and not m.penalty_get(1).any() and m.resident_bytes() == rb0
        m.penalty_set(1, None)                      # zeroing what does not exist allocates nothing either
        assert m.resident_bytes() == rb0
        c = np.array(nc.counts_of("a"), np.float32)
        m.penalty_set(1, c)
        assert m.resident_bytes() == rb0 + ROWS * V * 4
        assert np.array_equal(m.penalty_get(1), c) and not m.penalty_get(0).any() and not m.penalty_get(2).any()
        us = [nc.splitmix_u(77, k) for k in range(8)]
        for u in us:                                # without UPDATE the counts stay
            m.sample_nucleus(1.0, 0.9, 40, 0.4, 0.4, 0.996, u, slot=1)
        assert np.array_equal(m.penalty_get(1).view(np.uint32), c.view(np.uint32))
        for decay in (0.996, 1.0):
            for u in us:
                r = nc.reference(lg, 1.0, 0.9, 40, c, 0.4, 0.4)
                got = m.sample_nucleus(1.0, 0.9, 40, 0.4, 0.4, decay, u, slot=1, update=True)
                assert got == r.pick(u) or r.excused(u), (decay, u, got, r.pick(u))
                c = nc.count_update(c, got, decay)
            dev = m.penalty_get(1)
            print(f"decay {decay}: {int((dev > 0).sum())} counted ids, largest count {dev.max()!r}")
            assert np.array_equal(dev.view(np.uint32), c.view(np.uint32)), f"decay {decay}"
        assert not m.penalty_get(0).any() and not m.penalty_get(2).any() and not m.penalty_get(3).any()
    finally:
        m.close()


# ---- the generation loops on a model's own logits -------------------------------------------------------------------------------
L, D, N_GEN = 2, 256, 16
PEN = dict(presence=0.4, frequency=0.4, decay=0.996)
LOOPS = [dict(temp=1.0, top_p=0.9, top_k=40, **PEN), dict(temp=0.01, top_p=0.9, top_k=40, **PEN)]
LOOP_IDS = ["temp1", "temp0.01"]


@pytest.fixture(scope="module")
def model(eng):
    m = load(eng, L, D, 12, ROWS, head_scale=30.0)
    yield m
    m.close()


def follow(logits, counts, kw, u, got, where):
    """the reference's pick for this step (the device's where the draw is excused, and only there) and the counts behind it"""
    r = nc.reference(logits, kw["temp"], kw["top_p"], kw["top_k"], counts, kw["presence"], kw["frequency"], ban0=True)
    want = r.pick(u)
    if want != got:
        assert r.excused(u), f"{where}: device {got} reference {want} (u {u!r})"
        want = got
    return want, nc.count_update(counts, want, kw["decay"])


@pytest.mark.parametrize("kw", LOOPS, ids=LOOP_IDS)
def test_decode_nucleus_equals_the_reference_loop(model, kw):
    m, first, seed = model, 30000, 33
    m.reset_state()
    ids = [int(v) for v in m.decode_nucleus(first, N_GEN, seed=seed, **kw)]
    dev = m.penalty_get(0)
    print("decode_nucleus", kw, ids)
    m.reset_state()
    tk, c = first, np.zeros(V, np.float32)
    for step in range(N_GEN):
        logits = m.forward(tk)[:V].copy()
        tk, c = follow(logits, c, kw, nc.splitmix_u(seed, step), ids[step], f"step {step}")
    assert np.array_equal(dev.view(np.uint32), c.view(np.uint32))
    assert all(0 < v < V for v in ids)


@pytest.mark.parametrize("kw", LOOPS, ids=LOOP_IDS)
def test_decode_batch_nucleus_equals_the_reference_loop(eng, model, kw):
    m, first, seeds = model, [9, 4242, 30000], [11, 22, 33]
    m.reset_state()
    got = m.decode_batch_nucleus(first, N_GEN, seeds=seeds, **kw).astype(np.int64)
    dev = [m.penalty_get(s) for s in range(3)]
    print("decode_batch_nucleus", kw, got.tolist())
    m.reset_state()
    ids, cs = list(first), [np.zeros(V, np.float32) for _ in range(3)]
    for step in range(N_GEN):
        lg = m.forward(ids, eng.MODE_PARRALEL)[: 3 * V].reshape(3, V).copy()
        for s in range(3):
            ids[s], cs[s] = follow(lg[s], cs[s], kw, nc.splitmix_u(seeds[s], step), int(got[s, step]), f"stream {s} step {step}")
    for s in range(3):
        assert np.array_equal(dev[s].view(np.uint32), cs[s].view(np.uint32)), f"stream {s}"
    assert ((got > 0) & (got < V)).all()


def restated(ids, decay):
    c = np.zeros(V, np.float32)
    for g in ids:
        c = nc.count_update(c, int(g), decay)
    return c


def test_keep_continues_a_call_and_its_counts(model):
    m, first, seed, kw = model, 4242, 5, LOOPS[0]
    m.reset_state()
    whole = m.decode_nucleus(first, 16, seed=seed, **kw).tolist()
    c16 = m.penalty_get(0)
    m.reset_state()
    a = m.decode_nucleus(first, 8, seed=seed, **kw).tolist()            # (no KEEP: starts from zero counts although the call above left some)
    b = m.decode_nucleus(a[-1], 8, seed=seed + 8, keep=True, **kw).tolist()
    print("16:", whole, "8 + 8:", a, b)
    assert a + b == whole
    assert np.array_equal(m.penalty_get(0).view(np.uint32), c16.view(np.uint32))
    assert np.array_equal(c16.view(np.uint32), restated(whole, kw["decay"]).view(np.uint32))
    # without KEEP the second call starts from zero counts
    fresh = m.decode_nucleus(a[-1], 8, seed=seed + 8, **kw).tolist()
    assert np.array_equal(m.penalty_get(0).view(np.uint32), restated(fresh, kw["decay"]).view(np.uint32))


def test_keep_continues_a_batched_call(model):
    m, first, seeds, kw = model, [9, 4242, 30000], [11, 22, 33], LOOPS[0]
    m.reset_state()
    whole = m.decode_batch_nucleus(first, 16, seeds=seeds, **kw)
    c16 = [m.penalty_get(s) for s in range(3)]
    m.reset_state()
    a = m.decode_batch_nucleus(first, 8, seeds=seeds, **kw)
    b = m.decode_batch_nucleus(a[:, -1].tolist(), 8, seeds=[s + 8 for s in seeds], keep=True, **kw)
    assert np.array_equal(np.concatenate([a, b], axis=1), whole)
    for s in range(3):
        assert np.array_equal(m.penalty_get(s).view(np.uint32), c16[s].view(np.uint32))
        assert np.array_equal(c16[s].view(np.uint32), restated(whole[s], kw["decay"]).view(np.uint32))
    fresh = m.decode_batch_nucleus(a[:, -1].tolist(), 8, seeds=[s + 8 for s in seeds], **kw)
    for s in range(3):
        assert np.array_equal(m.penalty_get(s).view(np.uint32), restated(fresh[s], kw["decay"]).view(np.uint32))


# ---- the pybind module: RWKV::sampleNucleus / decodeNucleus of include/rwkv.h at run time, host-authoritative state (push / pull) ------
def test_pybind_nucleus_matches_the_python_engine(eng, rwkv_mod, tmp_path):
    rwkv = rwkv_mod
    path = str(tmp_path / "model.bin")
    mf.write_bin(path, L, 128, mf.synthetic_tensors(L, 128, seed=43, head_scale=30.0))
    kw = LOOPS[0]
    m = eng.RWKV()                                  # host state authoritative, as the module's RWKV object
    m.loadFile(path)
    want_a = m.decode_nucleus(30000, 8, seed=7, **kw).tolist()
    want_b = m.decode_nucleus(want_a[-1], 8, seed=15, keep=True, **kw).tolist()
    m.close()
    h = rwkv.initRwkv()
    rwkv.loadModel(h, path)
    rwkv.initOutput(h); rwkv.initState(h)
    got_a = [int(v) for v in rwkv.decodeNucleus(h, 30000, 8, kw["temp"], kw["top_p"], kw["top_k"], kw["presence"], kw["frequency"], kw["decay"], 7)]
    got_b = [int(v) for v in rwkv.decodeNucleus(h, got_a[-1], 8, seed=15, keep=True, **kw)]
    print("pybind decodeNucleus", got_a, got_b)
    assert got_a == want_a and got_b == want_b
    # nucleusSample draws from the logits of the last modelForward and counts its pick: top_k 1 is the penalised argmax whatever u is, and a
    # presence of 1000 takes every id counted so far (the sixteen picks above, then its own) out of the running
    rwkv.modelForward(h, got_b[-1])
    out = np.array(rwkv.getOutput(h), np.float32)
    out[[0] + got_a + got_b] = -np.inf
    for _ in range(3):
        pick = rwkv.nucleusSample(h, temp=1.0, top_p=1.0, top_k=1, presence=1000.0, ban0=True)
        assert pick == int(out.argmax())
        out[pick] = -np.inf
    rwkv.freeRwkv(h)


# ---- refused calls: one table in the style of tests/test_abi_guards_gpu.py ---------------------------------------------------------
GL, GD, MAXT = 2, 64, 8
u64 = C.c_uint64


def a64(*v):
    return (u64 * len(v))(*v)


def P(temp=1.0, top_p=0.9, top_k=40, presence=0.4, frequency=0.4, decay=0.996, flags=0, reserved=0):
    from rwkv_cpp_accelerated_amd import engine
    p = engine.nucleus_params(temp, top_p, top_k, presence, frequency, decay, flags)
    p.reserved = reserved
    return p


OK2, BAD2, NINE = a64(1, 2), a64(1, V), a64(*[1] * (MAXT + 1))
OUT = (u64 * 64)()
CNT = (C.c_float * V)()
NAN, INF = float("nan"), float("inf")
NOT_LOADED, WHOLE, HEAD, NULL = "RWKV not loaded", "whole-model", "hold the head", "NULL"
TOKEN = f"token id {V} out of range"

# (entry point, arguments -- "M" / "U" / "S" / "W" name a context, a dict stands for rwkv_nucleus_params --, status, a piece of the message)
GUARDS = [
    # ---- a NULL pointer ----
    ("rwkv_sample_nucleus", (None, 0, 0, {}, 0.5, OUT), E_ARG, NULL),
    ("rwkv_sample_nucleus", ("M", 0, 0, None, 0.5, OUT), E_ARG, NULL),
    ("rwkv_sample_nucleus", ("M", 0, 0, {}, 0.5, None), E_ARG, NULL),
    ("rwkv_decode_nucleus", (None, 1, 4, {}, 3, OUT), E_ARG, NULL),
    ("rwkv_decode_nucleus", ("M", 1, 4, None, 3, OUT), E_ARG, NULL),
    ("rwkv_decode_nucleus", ("M", 1, 4, {}, 3, None), E_ARG, NULL),
    ("rwkv_decode_batch_nucleus", (None, OK2, 2, 4, {}, OK2, OUT), E_ARG, NULL),
    ("rwkv_decode_batch_nucleus", ("M", None, 2, 4, {}, OK2, OUT), E_ARG, NULL),
    ("rwkv_decode_batch_nucleus", ("M", OK2, 2, 4, None, OK2, OUT), E_ARG, NULL),
    ("rwkv_decode_batch_nucleus", ("M", OK2, 2, 4, {}, None, OUT), E_ARG, NULL),
    ("rwkv_decode_batch_nucleus", ("M", OK2, 2, 4, {}, OK2, None), E_ARG, NULL),
    ("rwkv_penalty_set", (None, 0, CNT), E_ARG, NULL),
    ("rwkv_penalty_get", (None, 0, CNT), E_ARG, NULL),
    ("rwkv_penalty_get", ("M", 0, None), E_ARG, NULL),
    # ---- !(temp > 0) ----
    ("rwkv_sample_nucleus", ("M", 0, 0, dict(temp=0.0), 0.5, OUT), E_ARG, "temp > 0"),
    ("rwkv_sample_nucleus", ("M", 0, 0, dict(temp=NAN), 0.5, OUT), E_ARG, "temp > 0"),
    ("rwkv_decode_nucleus", ("M", 1, 4, dict(temp=-1.0), 3, OUT), E_ARG, "temp > 0"),
    ("rwkv_decode_batch_nucleus", ("M", OK2, 2, 4, dict(temp=0.0), OK2, OUT), E_ARG, "temp > 0"),
    ("rwkv_decode_batch_nucleus", ("M", OK2, 1, 4, dict(temp=0.0), OK2, OUT), E_ARG, "temp > 0"),
    # ---- a non-finite top_p, presence or frequency ----
    ("rwkv_sample_nucleus", ("M", 0, 0, dict(top_p=NAN), 0.5, OUT), E_ARG, "must be finite"),
    ("rwkv_sample_nucleus", ("M", 0, 0, dict(top_p=INF), 0.5, OUT), E_ARG, "must be finite"),
    ("rwkv_decode_nucleus", ("M", 1, 4, dict(presence=INF), 3, OUT), E_ARG, "must be finite"),
    ("rwkv_decode_batch_nucleus", ("M", OK2, 2, 4, dict(frequency=NAN), OK2, OUT), E_ARG, "must be finite"),
    # ---- decay outside [0, 1] ----
    ("rwkv_sample_nucleus", ("M", 0, 0, dict(decay=1.5), 0.5, OUT), E_ARG, "decay must be in [0, 1]"),
    ("rwkv_decode_nucleus", ("M", 1, 4, dict(decay=-0.1), 3, OUT), E_ARG, "decay must be in [0, 1]"),
    ("rwkv_decode_batch_nucleus", ("M", OK2, 2, 4, dict(decay=NAN), OK2, OUT), E_ARG, "decay must be in [0, 1]"),
    # ---- unknown flag bits, reserved != 0 ----
    ("rwkv_sample_nucleus", ("M", 0, 0, dict(flags=8), 0.5, OUT), E_ARG, "unknown flag bits"),
    ("rwkv_decode_nucleus", ("M", 1, 4, dict(flags=0x80000002), 3, OUT), E_ARG, "unknown flag bits"),
    ("rwkv_decode_batch_nucleus", ("M", OK2, 2, 4, dict(reserved=1), OK2, OUT), E_ARG, "reserved != 0"),
    ("rwkv_sample_nucleus", ("M", 0, 0, dict(reserved=7), 0.5, OUT), E_ARG, "reserved != 0"),
    # ---- u outside [0, 1) ----
    ("rwkv_sample_nucleus", ("M", 0, 0, {}, 1.0, OUT), E_ARG, "u < 1"),
    ("rwkv_sample_nucleus", ("M", 0, 0, {}, -0.5, OUT), E_ARG, "0 <= u"),
    ("rwkv_sample_nucleus", ("M", 0, 0, {}, NAN, OUT), E_ARG, "0 <= u"),
    # ---- a row or slot equal to max_ctx ----
    ("rwkv_sample_nucleus", ("M", MAXT, 0, {}, 0.5, OUT), E_ARG, "logits row 8 or slot 0 out of range"),
    ("rwkv_sample_nucleus", ("M", 0, MAXT, {}, 0.5, OUT), E_ARG, "logits row 0 or slot 8 out of range"),
    ("rwkv_penalty_set", ("M", MAXT, CNT), E_ARG, "slot 8 out of range"),
    ("rwkv_penalty_set", ("M", MAXT, None), E_ARG, "slot 8 out of range"),
    ("rwkv_penalty_get", ("M", MAXT, CNT), E_ARG, "slot 8 out of range"),
    # ---- a token id of 50277 ----
    ("rwkv_decode_nucleus", ("M", V, 4, {}, 3, OUT), E_ARG, TOKEN),
    ("rwkv_decode_batch_nucleus", ("M", BAD2, 2, 4, {}, OK2, OUT), E_ARG, TOKEN),
    ("rwkv_decode_batch_nucleus", ("M", a64(V), 1, 4, {}, OK2, OUT), E_ARG, TOKEN),
    # ---- a bad step or stream count ----
    ("rwkv_decode_nucleus", ("M", 1, 0, {}, 3, OUT), E_ARG, "n_tokens must be in 1..65536"),
    ("rwkv_decode_nucleus", ("M", 1, 65537, {}, 3, OUT), E_ARG, "n_tokens must be in 1..65536"),
    ("rwkv_decode_batch_nucleus", ("M", OK2, 0, 4, {}, OK2, OUT), E_ARG, "n_streams must be in 1..8"),
    ("rwkv_decode_batch_nucleus", ("M", NINE, MAXT + 1, 4, {}, NINE, OUT), E_ARG, "n_streams must be in 1..8"),
    ("rwkv_decode_batch_nucleus", ("M", OK2, 2, 0, {}, OK2, OUT), E_ARG, "n_steps must be in 1..65536"),
    ("rwkv_decode_batch_nucleus", ("M", OK2, 2, 65537, {}, OK2, OUT), E_ARG, "n_steps must be in 1..65536"),
    ("rwkv_decode_batch_nucleus", ("M", OK2, 1, 65537, {}, OK2, OUT), E_ARG, "n_steps must be in 1..65536"),
    # ---- RWKV_E_STATE as for the typical calls: not loaded, a stage context, two streams without the chunk path ----
    ("rwkv_sample_nucleus", ("U", 0, 0, {}, 0.5, OUT), E_STATE, NOT_LOADED),
    ("rwkv_decode_nucleus", ("U", 1, 4, {}, 3, OUT), E_STATE, NOT_LOADED),
    ("rwkv_decode_batch_nucleus", ("U", OK2, 2, 4, {}, OK2, OUT), E_STATE, NOT_LOADED),
    ("rwkv_penalty_set", ("U", 0, CNT), E_STATE, NOT_LOADED),
    ("rwkv_penalty_get", ("U", 0, CNT), E_STATE, NOT_LOADED),
    ("rwkv_sample_nucleus", ("S", 0, 0, {}, 0.5, OUT), E_STATE, HEAD),
    ("rwkv_decode_nucleus", ("S", 1, 4, {}, 3, OUT), E_STATE, WHOLE),
    ("rwkv_decode_batch_nucleus", ("S", OK2, 2, 4, {}, OK2, OUT), E_STATE, WHOLE),
    ("rwkv_decode_batch_nucleus", ("S", OK2, 1, 4, {}, OK2, OUT), E_STATE, WHOLE),
    ("rwkv_decode_batch_nucleus", ("W", OK2, 2, 4, {}, OK2, OUT), E_STATE, "needs the chunk path"),
    # ---- two faults at once: the first check in the entry point's order answers ----
    ("rwkv_sample_nucleus", ("U", MAXT, MAXT, None, 1.0, OUT), E_ARG, NULL),
    ("rwkv_sample_nucleus", ("S", MAXT, 0, dict(temp=0.0), 1.0, OUT), E_STATE, HEAD),
    ("rwkv_sample_nucleus", ("M", MAXT, 0, dict(temp=0.0), 1.0, OUT), E_ARG, "out of range"),
    ("rwkv_sample_nucleus", ("M", 0, 0, dict(temp=0.0), 1.0, OUT), E_ARG, "temp > 0"),
    ("rwkv_decode_nucleus", ("M", V, 0, dict(temp=0.0), 3, OUT), E_ARG, TOKEN),
    ("rwkv_decode_nucleus", ("M", 1, 0, dict(temp=0.0), 3, OUT), E_ARG, "n_tokens must be in"),
    ("rwkv_decode_batch_nucleus", ("M", BAD2, 2, 4, dict(decay=2.0), OK2, OUT), E_ARG, TOKEN),
]


def _guard_id(i):
    entry, args = GUARDS[i][0], GUARDS[i][1]
    return f"{i:02d}-{entry[5:]}-{args[0] if isinstance(args[0], str) else 'null'}"


@pytest.fixture(scope="module")
def gctx(eng):
    x = GuardContexts(eng, GL, GD, MAXT, extra=("W",), counts=[np.roll(nc.counts_of("a"), 1000 * s) for s in range(MAXT)])
    yield x
    x.close()


@pytest.mark.parametrize("i", range(len(GUARDS)), ids=_guard_id)
def test_a_refused_call_answers_its_status_and_launches_nothing(gctx, i):
    entry, args, status, text = GUARDS[i]
    keep = [P(**v) if isinstance(v, dict) else None for v in args]
    call = [gctx.h[v] if isinstance(v, str) else C.byref(k) if isinstance(v, dict) else v for v, k in zip(args, keep)]
    check_refused(gctx, entry, call, status, text)
