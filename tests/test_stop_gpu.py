"""Stop sequences and per-stream budgets in the device decode loops (rwkv_decode_batch_until, csrc/stop.hip.h) on the synthetic model of
test_batch_decode_gpu.py.  Planted picks through rwkv_debug_stop_scan against the restatement of tests/stop_cases.py; model runs against
the plain rwkv_decode_batch_* calls: the picks, and for every length the state, logits row and counts that the plain call of that many
steps leaves.  Every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

from rwkv_cpp_accelerated_amd import modelfile as mf
import stop_cases as sc
from support import E_ARG, E_STATE, build_app, eng, firsts_of, load, restore, run_app, seeds_of, slots, start_state  # noqa: F401

pytestmark = pytest.mark.gpu

L, D, MAXN, STEPS = 3, 256, 96, sc.STEPS
NUC = dict(temp=1.0, top_p=0.9, presence=0.4, frequency=0.4, decay=0.996)      # nucleus with penalties: the counts are part of a slot
KINDS = ["greedy", "typical", "nucleus"]


@pytest.fixture(scope="module")
def tensors():
    return mf.synthetic_tensors(L, D, seed=21, head_scale=30.0)


@pytest.fixture(scope="module")
def model(eng, tensors):
    m = load(eng, L, D, 21, MAXN, tensors)
    yield m
    m.close()


@pytest.fixture(scope="module")
def start(eng, model):
    """distinct state in every slot: where every run of this module starts"""
    return start_state(eng, model, MAXN)


def plain(m, kind, first, steps, seeds, keep=False):
    if kind == "greedy":
        return m.decode_batch_greedy(first, steps).astype(np.int64)
    if kind == "typical":
        return m.decode_batch_typical(first, steps, temp=0.45, tau=0.8, seeds=seeds).astype(np.int64)
    return m.decode_batch_nucleus(first, steps, seeds=seeds, keep=keep, **NUC).astype(np.int64)


def until(m, kind, first, steps, seeds, stops=(), max_new=None, keep=False):
    kw = dict(greedy={}, typical=dict(temp=0.45, tau=0.8), nucleus=NUC)[kind]
    ids, ln, rs, ran = m.decode_batch_until(first, steps, stops=stops, max_new=max_new, keep=keep, pick=kind, seeds=seeds, **kw)
    return ids.astype(np.int64), ln, rs, ran


def stops_from(U, first, which):
    """stop sequences taken from the unstopped ids: one single id, one pair, one 8-gram and (which = 1) one pair that starts at first[s]"""
    n = len(U)
    a, b, c, d = (0, 2, 5, n - 1) if n > 5 else (0, 0, 0, 0)       # streams without a budget (s % 3 != 1)
    stops = [[int(U[a][5])], [int(v) for v in U[b][9:11]], [int(v) for v in U[c][10:18]]]
    if which:
        stops.append([int(first[d]), int(U[d][0])])
    return stops


def check_against_plain(m, start, kind, n, U, first, seeds, stops, max_new):
    """run the stopped call from `start`; lengths, reasons and ids against the restatement on U; every slot against the plain call of its length"""
    want_len, want_reason = sc.scan_all(U, first, stops, max_new)
    restore(m, start)
    ids, ln, rs, ran = until(m, kind, first, STEPS, seeds, stops, max_new)
    got = slots(m, n, kind == "nucleus")
    print(f"{kind} n={n}: len {ln.tolist()} reason {rs.tolist()} steps_run {ran}")
    assert np.array_equal(ln, want_len) and np.array_equal(rs, want_reason)
    assert ran <= sc.bound(int(ln.max()), STEPS)
    for s in range(n):
        assert np.array_equal(ids[s][: ln[s]], U[s][: ln[s]]) and not ids[s][ln[s]:].any(), s
    for l in sorted(set(int(v) for v in ln)):
        restore(m, start)
        assert np.array_equal(plain(m, kind, first, l, seeds), U[:, :l])
        ref = slots(m, n, kind == "nucleus")
        at = np.flatnonzero(ln == l)
        for g, r in zip(got, ref):
            assert np.array_equal(g[at], r[at]), (l, at.tolist())
    return ln, rs


# ---- planted picks: k_stop_step alone ----

@pytest.mark.parametrize("name", list(sc.PLANTED))
def test_planted_strings(model, name):
    call = sc.PLANTED[name]
    firsts = [st[0] for st in call["streams"]]
    ids = np.array([st[1] for st in call["streams"]], np.int64)
    max_new = [st[2] for st in call["streams"]]
    max_new = None if all(v is None for v in max_new) else [STEPS if v is None else v for v in max_new]
    ln, rs = model.debug_stop_scan(ids, firsts, call["stops"], max_new)
    want = sc.scan_all(ids, firsts, call["stops"], max_new)
    assert np.array_equal(ln, want[0]) and np.array_equal(rs, want[1]), (ln, rs, want)


def test_planted_96_streams(model):
    ids, firsts, stops, max_new = sc.many_streams(MAXN)
    ln, rs = model.debug_stop_scan(ids, firsts, stops, max_new)
    want = sc.scan_all(ids, firsts, stops, max_new)
    assert np.array_equal(ln, want[0]) and np.array_equal(rs, want[1])
    assert (rs >= 2).sum() >= 30 and (rs == 1).sum() >= 3 and len(set(ln.tolist())) >= 8


def test_planted_keep_across_a_split_at_every_position(model):
    firsts, ids = sc.keep_streams()
    full = sc.scan_all(ids, firsts, [sc.KEEP_SEQ])
    assert full[0].tolist() == [16, 15, 14, 13] and full[1].tolist() == [2] * 4
    ln, rs = model.debug_stop_scan(ids[:, :12], firsts, [sc.KEEP_SEQ])
    assert ln.tolist() == [12] * 4 and rs.tolist() == [0] * 4
    ln, rs = model.debug_stop_scan(ids[:, 12:], ids[:, 11], [sc.KEEP_SEQ], keep=True)
    assert (12 + ln).tolist() == full[0].tolist() and rs.tolist() == [2] * 4
    # without KEEP the second call starts from its first token alone: only the stream whose sequence lies wholly behind the split matches,
    # and the one that holds all of it but its first id in the second call with that id as first_token
    model.debug_stop_scan(ids[:, :12], firsts, [sc.KEEP_SEQ])
    ln, rs = model.debug_stop_scan(ids[:, 12:], ids[:, 11], [sc.KEEP_SEQ])
    assert rs.tolist() == [2, 2, 0, 0] and ln.tolist() == [4, 3, 12, 12]


def test_planted_keep_after_a_foreign_first_token_restarts(model):
    a, b, c, z = sc.A, sc.B, sc.C_, sc.Z
    stops = [[a, b, c]]
    model.debug_stop_scan(np.array([sc.pad([z, a, b], 12)] * 2), [z, z], stops)           # both histories end in ... a b z z z
    model.debug_stop_scan(np.array([sc.pad([z, a, b], 3)] * 2), [z, z], stops)            # both end in a b
    # stream 0 goes on from b; stream 1 was fed something else in between and comes back with a foreign first token
    ln, rs = model.debug_stop_scan(np.array([sc.pad([c], 6), sc.pad([b, c], 6)]), [b, a], stops, keep=True)
    assert (ln.tolist(), rs.tolist()) == ([1, 2], [2, 2])
    model.debug_stop_scan(np.array([sc.pad([z, a, b], 3)] * 2), [z, z], stops)
    ln, rs = model.debug_stop_scan(np.array([sc.pad([c], 6), sc.pad([c], 6)]), [b, z], stops, keep=True)
    assert (ln.tolist(), rs.tolist()) == ([1, 6], [2, 0])                                  # the restarted history holds no a b


# ---- model runs ----

@pytest.fixture(scope="module")
def unstopped(model, start):
    """U per (kind, n): the ids of the plain 24-step call, computed once"""
    cache = {}

    def get(kind, n):
        if (kind, n) not in cache:
            restore(model, start)
            cache[kind, n] = plain(model, kind, firsts_of(n), STEPS, seeds_of(n))
        return cache[kind, n]
    return get


@pytest.mark.parametrize("n", [1, 12, 70])
@pytest.mark.parametrize("kind", KINDS)
def test_stopped_streams_are_what_the_plain_call_leaves(model, start, unstopped, kind, n):
    U, first, seeds = unstopped(kind, n), firsts_of(n), seeds_of(n)
    budgets = [1 + s % 5 if s % 3 == 1 else STEPS for s in range(n)]
    seen = set()
    for which in (0, 1):
        stops = stops_from(U, first, which)
        ln, rs = check_against_plain(model, start, kind, n, U, first, seeds, stops, budgets if n > 1 or which else None)
        seen |= set(rs.tolist())
    if n > 1:
        assert 1 in seen and len([r for r in seen if r >= 2]) >= 3        # budgets and several sequences did stop streams
    else:
        assert seen & {2, 5}
        check_against_plain(model, start, kind, 1, U, first, seeds, [], [3])          # one stream, budget alone


def test_nothing_stops(model, start, unstopped):
    n = 12
    first, seeds = firsts_of(n), seeds_of(n)
    for kind in KINDS:
        U = unstopped(kind, n)
        restore(model, start)
        assert np.array_equal(plain(model, kind, first, STEPS, seeds), U)
        ref = slots(model, n, kind == "nucleus")
        absent = [v for v in range(1, 200) if v not in set(U.ravel().tolist())][:2]
        for stops, max_new in (([], None), ([absent, absent[:1] * 8], [STEPS] * n)):     # the plain loop; the stop kernels with nothing to find
            restore(model, start)
            ids, ln, rs, ran = until(model, kind, first, STEPS, seeds, stops, max_new)
            assert np.array_equal(ids, U) and ln.tolist() == [STEPS] * n and rs.tolist() == [0] * n and ran == STEPS
            for g, r in zip(slots(model, n, kind == "nucleus"), ref):
                assert np.array_equal(g, r)


def test_run_ahead_is_bounded(model, start, unstopped):
    n, kind, long = 12, "greedy", 4096
    U, first = unstopped(kind, n), firsts_of(n)
    budgets = [1 + s for s in range(n)]                       # everything has stopped by step 12
    restore(model, start)
    ids24, ln24, rs24, ran24 = until(model, kind, first, STEPS, None, [], budgets)
    ref = slots(model, n, False)
    restore(model, start)
    ids, ln, rs, ran = until(model, kind, first, long, None, [], budgets)
    print(f"steps_run {ran} of {long} (24-step call: {ran24})")
    assert ran <= sc.bound(12, long) == 24 and ran24 <= 24
    assert np.array_equal(ln, ln24) and ln.tolist() == budgets and rs.tolist() == [1] * n
    assert np.array_equal(ids[:, :STEPS], ids24) and not ids[:, STEPS:].any()
    for s in range(n):
        assert np.array_equal(ids[s][: ln[s]], U[s][: ln[s]])
    for g, r in zip(slots(model, n, False), ref):
        assert np.array_equal(g, r)
    # one stream on the decode kernels
    restore(model, start)
    ids, ln, rs, ran = until(model, kind, first[:1], long, None, [], [5])
    assert ran <= sc.bound(5, long) == 16 and ln.tolist() == [5] and rs.tolist() == [1]


def test_8_plus_8_with_keep_is_16(model, start):
    n, kind = 12, "nucleus"
    first, seeds = firsts_of(n), seeds_of(n)
    restore(model, start)
    U = plain(model, kind, first, 16, seeds)
    stops = [[int(U[2][7]), int(U[2][8])], [int(v) for v in U[5][5:11]], [int(U[7][12])]]      # two sequences lie across the boundary
    want = sc.scan_all(U, first, stops)
    restore(model, start)
    ids, ln, rs, _ = until(model, kind, first, 16, seeds, stops)
    full = slots(model, n, True)
    assert np.array_equal(ln, want[0]) and np.array_equal(rs, want[1])
    restore(model, start)
    ids1, ln1, rs1, _ = until(model, kind, first, 8, seeds, stops)
    ids2, ln2, rs2, _ = until(model, kind, [int(v) for v in ids1[:, 7]], 8, [s + 8 for s in seeds], stops, keep=True)
    halves = slots(model, n, True)
    on = np.flatnonzero(rs1 == 0)                       # the streams that the first call did not stop: the identity is about them
    assert len(on) >= 8 and {2, 5} <= set(on.tolist()) and ln[2] > 8 and ln[5] > 8
    assert np.array_equal(8 + ln2[on], ln[on]) and np.array_equal(rs2[on], rs[on])
    assert np.array_equal(np.concatenate([ids1, ids2], axis=1)[on], ids[on])
    for g, r in zip(halves, full):
        assert np.array_equal(g[on], r[on])


@pytest.mark.parametrize("kind", ["greedy", "nucleus"])
def test_a_stopped_stream_continues_from_its_last_token(model, start, unstopped, kind):
    n, more = 12, 4
    U, first, seeds = unstopped(kind, n), firsts_of(n), seeds_of(n)
    budgets = [2 + s for s in range(n)]
    restore(model, start)
    ids, ln, rs, _ = until(model, kind, first, STEPS, seeds, [[int(U[0][1])]], budgets)
    nxt = plain(model, kind, [int(ids[s][ln[s] - 1]) for s in range(n)], more, [seeds[s] + int(ln[s]) for s in range(n)], keep=True)
    for s in range(n):
        assert np.array_equal(nxt[s], U[s][ln[s]: ln[s] + more]), s


def test_rejected_calls_leave_everything_alone(eng, model, start, tensors):
    lib, m, n = eng.lib(), model, 4
    u64, u32 = C.c_uint64, C.c_uint32
    a, b, c, z = sc.A, sc.B, sc.C_, sc.Z
    restore(m, start)
    plain(m, "nucleus", firsts_of(n), 3, seeds_of(n))                                       # counts and logits hold something
    m.debug_stop_scan(np.array([sc.pad([z, a, b], 3)] * n), [z] * n, [[a, b, c]])        # the histories end in a b
    before = slots(m, n, True)
    ft, seeds, out, ln = (u64 * n)(*firsts_of(n)), (u64 * n)(*seeds_of(n)), (u64 * (n * 8))(), (u32 * n)()
    good_pick = eng.Pick(eng.PICK_NUCLEUS, 1.0, 0.8, 0, eng.nucleus_params(**NUC))

    def call(pick=good_pick, stops=((a, b),), max_new=None, flags=None, reserved=0, first=ft, n_=n, steps=8, sd=seeds, o=out, l=ln, raw=None):
        p, alive = eng.stop_params(stops, max_new)
        if flags is not None:
            p.flags = flags
        p.reserved = reserved
        if raw:
            raw(p)
        return int(lib.rwkv_decode_batch_until(m._h, first, n_, steps, C.byref(pick) if pick else None, sd, C.byref(p), o, l, None, None))

    bad = [call(pick=eng.Pick(3, 1.0, 0.8, 0, eng.nucleus_params())), call(pick=eng.Pick(-1, 1.0, 0.8, 0, eng.nucleus_params())),
           call(pick=None), call(l=None), call(o=None), call(first=None), call(sd=None),
           int(lib.rwkv_decode_batch_until(m._h, ft, n, 8, C.byref(good_pick), seeds, None, out, ln, None, None)),
           call(n_=0), call(n_=MAXN + 1), call(steps=0), call(steps=65537), call(first=(u64 * n)(1, 2, mf.VOCAB, 3)),
           call(pick=eng.Pick(eng.PICK_TYPICAL, 0.0, 0.8, 0, eng.nucleus_params())),
           call(pick=eng.Pick(eng.PICK_NUCLEUS, 1.0, 0.8, 0, eng.nucleus_params(decay=2.0))),
           call(stops=[(a,)] * 17), call(stops=[(a,) * 9]), call(stops=[(a, mf.VOCAB)]),
           call(raw=lambda p: setattr(p, "seq_ids", None)), call(raw=lambda p: setattr(p, "seq_len", None)),
           call(raw=lambda p: p.seq_len.__setitem__(0, 0)),
           call(max_new=[1, 0, 1, 1]), call(max_new=[1, 9, 1, 1]), call(flags=2), call(flags=1 | 4), call(reserved=1)]
    assert bad == [E_ARG] * len(bad), bad
    ids = np.zeros((n, 8), np.uint64)
    scan_bad = [int(lib.rwkv_debug_stop_scan(m._h, ids.ctypes.data_as(C.POINTER(u64)), ft, n, 8, C.byref(eng.stop_params([(a,) * 9])[0]), ln, ln)),
                int(lib.rwkv_debug_stop_scan(m._h, None, ft, n, 8, C.byref(eng.stop_params([(a,)])[0]), ln, ln)),
                int(lib.rwkv_debug_stop_scan(m._h, ids.ctypes.data_as(C.POINTER(u64)), ft, MAXN + 1, 8, C.byref(eng.stop_params([(a,)])[0]), ln, ln))]
    assert scan_bad == [E_ARG] * 3
    for g, r in zip(slots(m, n, True), before):
        assert np.array_equal(g, r)
    got = m.debug_stop_scan(np.array([sc.pad([c], 4)] * n), [b] * n, [[a, b, c]], keep=True)   # the histories still end in a b
    assert got[0].tolist() == [1] * n and got[1].tolist() == [2] * n
    # not loaded; a pipeline stage (no head); the chunk path off (one stream runs, two do not)
    e = eng.RWKV(resident=True)
    sp, _alive = eng.stop_params([(a, b)])
    args = lambda h, n_: (h, ft, n_, 8, C.byref(good_pick), seeds, C.byref(sp), out, ln, None, None)
    assert lib.rwkv_decode_batch_until(*args(e._h, 2)) == E_STATE
    assert lib.rwkv_debug_stop_scan(e._h, ids.ctypes.data_as(C.POINTER(u64)), ft, n, 8, C.byref(sp), ln, ln) == E_STATE
    e.close()
    e = eng.RWKV(resident=True)
    e.set_layer_range(0, 2)
    e.loadTensors(L, D, tensors, maxGPT=4)
    assert lib.rwkv_decode_batch_until(*args(e._h, 1)) == E_STATE
    e.close()
    os.environ["RWKV_SEQ"] = "0"
    try:
        e = eng.RWKV(resident=True)
        e.loadTensors(L, D, tensors, maxGPT=4)
    finally:
        del os.environ["RWKV_SEQ"]
    assert lib.rwkv_decode_batch_until(*args(e._h, 2)) == E_STATE
    assert lib.rwkv_decode_batch_until(*args(e._h, 1)) == 0
    e.close()


def test_the_park_buffer_is_counted_and_only_a_stopping_call_allocates_it(eng, tensors):
    m = eng.RWKV(resident=True)
    m.loadTensors(L, D, tensors, maxGPT=8)
    n = 4
    m.decode_batch_until(firsts_of(n), 8)                           # cannot stop a stream: the plain loop
    base = m.resident_bytes()
    m.decode_batch_greedy(firsts_of(n), 8)
    assert m.resident_bytes() == base
    m.decode_batch_until(firsts_of(n), 8, max_new=[8] * n)
    park = 4 * n * (10 * L * D + 50280)
    assert m.resident_bytes() - base == park + 4 * (5 * n + 2) + 4 * 8 * 8       # park buffer, run record, histories of max_ctx slots
    m.close()


def test_host_authoritative_mode(eng, tensors, start):
    m = eng.RWKV(resident=False)
    m.loadTensors(L, D, tensors, maxGPT=8)
    n = 6
    for a, s in zip(m.state.arrays(), start):
        a[:] = s.view(np.float64)[:8].ravel()
    first = firsts_of(n)
    ids, ln, rs, _ = m.decode_batch_until(first, 8, max_new=[1 + s for s in range(n)])
    dev = [np.zeros(8 * L * D) for _ in range(5)]
    assert eng.lib().rwkv_get_output(m._h, None, *[C.c_void_p(a.ctypes.data) for a in dev], 8) == 0
    for h, d in zip(m.state.arrays(), dev):
        assert np.array_equal(h[: n * L * D], d[: n * L * D])
    assert ln.tolist() == [1 + s for s in range(n)]
    m.close()


# ---- the C++ drop-in header ----

def test_stop_app_matches_python_engine(built, tmp_path):
    from rwkv_cpp_accelerated_amd import engine
    exe = build_app("stop_app", tmp_path)
    Lm, Dm, n, steps = 2, 256, 5, 16
    t = mf.synthetic_tensors(Lm, Dm, seed=31, head_scale=30.0)
    p = str(tmp_path / "model.bin")
    mf.write_bin(p, Lm, Dm, t)
    m = engine.RWKV(resident=True)
    m.loadFile(p, n)
    first = [100 + s for s in range(n)]

    def prefill():
        m.reset_state()
        m.forward([5, 6, 7], engine.MODE_GPT)
        for s in range(1, n):
            m.copy_state(s, 0)

    prefill()
    U = m.decode_batch_nucleus(first, steps, seeds=list(range(n)), **NUC).astype(np.int64)
    stop = [int(U[1][3]), int(U[1][4])]
    budgets = [steps, steps, 3, steps, 7]
    rc, lines, raw = run_app(exe, [p, n, steps, *budgets, "--", *stop])
    assert rc == 0, raw
    assert lines[-1] == "stop_ok"
    rows = np.array([[int(x) for x in l.split()] for l in lines[-1 - n:-1]], np.int64)          # per stream: len reason ids...
    prefill()
    ids, ln, rs, _ = m.decode_batch_until(first, steps, stops=[stop], max_new=budgets, pick="nucleus", seeds=list(range(n)), **NUC)
    assert np.array_equal(rows[:, 0], ln) and np.array_equal(rows[:, 1], rs) and np.array_equal(rows[:, 2:], ids.astype(np.int64))
    assert rs[1] == 2 and (rs == 1).any()
    m.close()
