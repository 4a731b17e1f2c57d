"""Speculative greedy decoding on the device (include/rwkv_mi355x.h rwkv_spec_verify / rwkv_decode_speculative, csrc/spec.hip.h and the CKPT
instances of csrc/seq.hip.h): the rollback is EXACT.  The reference is rwkv_forward alone -- growing prefixes of at least two rows from a saved
non-zero start state, picked by the rule of tests/spec_cases.py -- and the verify's state, logits rows 0 .. a and ids are held to it bit for bit;
for a = 0, where rwkv_forward of one row runs the decode kernels, the verify is held bit for bit to rwkv_spec_verify(n_draft = 0) and to the
oracle within the chunk suite's bounds (3e-5 of the vector's max |.| for xy / dd, 1e-4 for aa / bb).  Every context has max_ctx = 34."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from rwkv_cpp_accelerated_amd import modelfile as mf
import parity
import spec_cases as sc
from support import E_ARG, E_STATE, NAMES, build_app, eng, load, restore, rows, same_state, snapshot  # noqa: F401

pytestmark = pytest.mark.gpu
V, MAXT = sc.V, sc.MAXT
TOKEN = 4242                                 # the id fed first in the width cases


class Width:
    """one model of the width cases with its start state and the reference continuation g, built with rwkv_forward alone (once per module)"""

    def __init__(self, eng, L, D):
        self.L, self.D = L, D
        self.t = mf.synthetic_tensors(L, D, seed=sc.SEED + D)
        self.m = load(eng, L, D, 0, MAXT, self.t)
        m = self.m
        rng = np.random.default_rng(D)
        m.forward([int(v) for v in rng.integers(1, V, MAXT)], eng.MODE_PARRALEL)     # a history on every slot
        m.forward([7, 50000, 11, 9], eng.MODE_GPT)                                    # and a prompt on slot 0
        self.start = snapshot(m, MAXT)
        # g[i] = the pick of row i of forward([TOKEN, g[0 .. i - 1]]); the state and the rows that forward of a + 1 >= 2 rows leaves
        self.g, self.state, self.rows = [], {}, {}
        restore(m, self.start)
        m.forward([TOKEN, 1], eng.MODE_GPT)
        self.g.append(sc.pick(m.logits(1)))
        for a in range(1, sc.MAX_DRAFT + 1):
            restore(m, self.start)
            m.forward([TOKEN] + self.g[:a], eng.MODE_GPT)
            self.state[a] = snapshot(m, MAXT)
            self.rows[a] = rows(m, a + 1)
            self.g.append(sc.pick(m.logits(a + 1)[a * V:]))
        for a in self.state:
            for x in self.state[a] + [self.rows[a]]:
                x.setflags(write=False)

    def close(self):
        self.m.close()


@pytest.fixture(scope="module")
def widths(eng):
    cache = {}

    def get(L, D):
        if (L, D) not in cache:
            cache[(L, D)] = Width(eng, L, D)
        return cache[(L, D)]
    yield get
    for w in cache.values():
        w.close()


@pytest.mark.parametrize("n_draft", sc.N_DRAFTS)
@pytest.mark.parametrize("L,D", sc.WIDTHS)
def test_rollback_is_exact(eng, widths, L, D, n_draft):
    w = widths(L, D)
    m = w.m
    restore(m, w.start)
    assert m.spec_verify(TOKEN, []) == (0, w.g[0])                   # n_draft = 0: a plain step on the chunk path
    zero, zero_row = snapshot(m, MAXT), rows(m, 1)
    for label, d, a_want in sc.planted(w.g, n_draft):
        restore(m, w.start)
        a, nx = m.spec_verify(TOKEN, d)
        what = f"D{D} n_draft {n_draft} wrong id {label}"
        assert (a, nx) == (a_want, w.g[a_want]), what
        got = snapshot(m, MAXT)
        same_state(got, w.start, what + ", slots 1 .. 33", slice(1, None))
        if a >= 1:
            same_state(got, w.state[a], what)
            assert np.array_equal(rows(m, a + 1), w.rows[a]), what + ": logits rows 0 .. a"
        else:
            same_state(got, zero, what + " against n_draft = 0")
            assert np.array_equal(rows(m, 1), zero_row), what + ": logits row 0"


@pytest.mark.parametrize("L,D", sc.WIDTHS)
def test_one_row_pass_is_within_the_chunk_bounds_of_the_oracle(eng, oracle, widths, L, D):
    """a = 0 is the one-row pass of the chunk path (rwkv_forward of one row runs the decode kernels): held to the oracle within the chunk suite's
    bounds, 3e-5 of the vector's max |.| for xy / dd and 1e-4 for aa / bb, layer by layer"""
    w = widths(L, D)
    m = w.m
    restore(m, w.start)
    assert m.spec_verify(TOKEN, []) == (0, w.g[0])
    zero, zero_row = snapshot(m, MAXT), rows(m, 1)
    om = oracle.from_tensors(L, D, w.t)
    st = [s.view(np.float64)[0].copy() for s in w.start]
    ref = om.forward([TOKEN], st)
    om.close()
    for l in range(L):
        lo = slice(l * D, (l + 1) * D)
        for k, tol in ((0, parity.TOL), (1, 1e-4), (2, 1e-4), (4, parity.TOL)):
            e = parity._close(zero[k].view(np.float64)[0][lo], st[k][lo], f"D{D} a = 0, layer {l} state {NAMES[k]}", tol)
            print(f"D{D} a = 0 layer {l} {NAMES[k]}: {e:.2e}")
    assert np.array_equal(zero[3], w.start[3])                       # pp: the chunk path does not use it
    parity.check_logits(zero_row[0].view(np.float32), ref[0], f"D{D} a = 0 logits")


@pytest.mark.parametrize("L,D", sc.WIDTHS[:3])
def test_three_verifies_chain_like_one_forward(eng, widths, L, D):
    w = widths(L, D)
    m, g = w.m, w.g
    restore(m, w.start)
    d = g[:5]
    d[2] = sc.wrong(d[2])
    assert m.spec_verify(TOKEN, d) == (2, g[2])                      # consumed TOKEN, g[0], g[1]
    assert m.spec_verify(g[2], g[3:7]) == (4, g[7])                  # g[2] .. g[6], all of the draft stands
    assert m.spec_verify(g[7], [sc.wrong(g[8])]) == (0, g[8])      # g[7]
    same_state(snapshot(m, MAXT), w.state[8], f"D{D} after three verifies")     # = forward([TOKEN] + g[:8]) from the start state


def test_draft_ids_at_the_edges(eng, widths):
    L, D = sc.WIDTHS[0]
    w = widths(L, D)
    m, g = w.m, w.g
    assert 0 not in g[:8] and V - 1 not in g[:8]
    for planted_id in (0, V - 1):                                    # the pick is never 0, and not 50276 here: the draft stops there
        for p in (0, 2, 3):
            d = g[:4]
            d[p] = planted_id
            restore(m, w.start)
            assert m.spec_verify(TOKEN, d) == (p, g[p]), (planted_id, p)
    # a model whose every row picks 50276 (the last id of the vocabulary): a draft of that id is accepted exactly as far as it says so
    e = load(eng, L, D, 0, MAXT, sc.edge_tensors(L, D, sc.SEED))
    e.forward([5, 6], eng.MODE_GPT)
    st = snapshot(e, MAXT)
    for d, a_want in (([V - 1] * 5, 5), ([V - 1, V - 1, 7, V - 1], 2), ([V - 2, V - 1], 0), ([V - 1] * 31, 31)):
        restore(e, st)
        assert e.spec_verify(9, d) == (a_want, V - 1), d
    e.close()


@pytest.fixture(scope="module")
def trio(eng):
    """the loop's target (3 x 320), a second context with the same weights, a narrower draft of another seed, and the reference ids"""
    L, D = 3, 320
    t = mf.synthetic_tensors(L, D, seed=sc.SEED + 1)
    target, same, other = load(eng, L, D, 0, MAXT, t), load(eng, L, D, 0, MAXT, t), load(eng, 3, 64, sc.SEED + 2, MAXT)
    prompt = [5, 6, 7, 800, 9]
    for m in (target, same, other):
        m.forward(prompt, eng.MODE_GPT)
    start = {m: snapshot(m, MAXT) for m in (target, same, other)}
    ids, t_ = [], 100
    for _ in range(60):                                              # repeated spec_verify(n_draft = 0): the continuation every loop must give
        t_ = target.spec_verify(t_, [])[1]
        ids.append(t_)
    # a drafter that is right EXCEPT where the continuation holds one of a few ids: the target's weights with those ids' columns of the head at 0
    # (it cannot pick them; everything in front of the head, and so its state under the same ids, is the target's)
    banned = sorted({ids[j] for j in PART_WRONG_AT})
    tp = list(t)
    h = tp[mf.HEAD].reshape(D, V).copy()
    h[:, banned] = 0
    tp[mf.HEAD] = h.reshape(-1)
    part = load(eng, L, D, 0, MAXT, tp)
    part.forward(prompt, eng.MODE_GPT)
    start[part] = snapshot(part, MAXT)
    yield dict(target=target, same=same, other=other, part=part, banned=banned, start=start, ids=ids, first=100)
    for m in (target, same, other, part):
        m.close()


PART_WRONG_AT = (2, 7, 8, 13, 20, 21, 22, 30, 41)      # positions of the continuation whose ids the "part" drafter cannot pick


def part_stats(ids, banned, first, n_tokens, k):
    """what the loop's statement (spec_cases.loop) counts for a drafter that guesses the continuation but for the banned ids, where it guesses
    something else and is lost for the rest of the round"""
    def draft(hist, kd):
        d = list(ids[len(hist) - 1:len(hist) - 1 + kd])
        for i, t in enumerate(d):
            if t in banned:
                return d[:i] + [0] * (kd - i)
        return d

    def verify(tok, d):
        pos = verify.pos
        a = sc.accept(d, ids[pos:pos + len(d) + 1])
        verify.pos = pos + a + 1
        return a, ids[pos + a]
    verify.pos = 0
    out, stats = sc.loop(verify, draft, first, n_tokens, k)
    assert out == ids[:n_tokens]
    return stats


def after_forward(eng, m, start, toks):
    """the state `m` holds after rwkv_forward of toks from its start state (pieces of <= 32 rows, at least 2 each)"""
    restore(m, start)
    toks = list(toks)
    while toks:
        n = len(toks) if len(toks) <= 32 else (32 if len(toks) != 33 else 31)
        m.forward(toks[:n], eng.MODE_GPT)
        toks = toks[n:]
    return snapshot(m, MAXT)


@pytest.mark.parametrize("k", [1, 4, 31])
@pytest.mark.parametrize("draft", ["same", "other", "part", "lookup"])
def test_loop_does_not_depend_on_the_draft(eng, trio, draft, k):
    target, ids, first = trio["target"], trio["ids"], trio["first"]
    dm = trio.get(draft)
    N = 48

    def run(tok, n, hist):
        return target.decode_lookup(hist + [tok], n, k=k, n=2) if dm is None else target.decode_speculative(dm, tok, n, k)

    def reset():
        restore(target, trio["start"][target])
        if dm is not None:
            restore(dm, trio["start"][dm])

    reset()
    got, stats = run(first, N, [])
    assert got.tolist() == ids[:N], draft
    print(f"draft {draft} k {k}: rounds {stats['rounds']} drafted {stats['drafted']} accepted {stats['accepted']}"
          f" acceptance {stats['accepted'] / max(1, stats['drafted']):.3f}")
    assert stats["accepted"] <= stats["drafted"] and stats["rounds"] <= N
    if draft == "part":                                              # rounds that end in the middle of the draft: 0 < a < k'
        assert stats == part_stats(ids, trio["banned"], first, N, k), stats
        assert 0 < stats["accepted"] < stats["drafted"] and (k == 1 or stats["rounds"] * (k + 1) > N + k)
    assert sc.pick(target.logits(1)) == ids[N - 1]                   # the row the last id was picked from is row 0
    fed = [first] + ids[:N - 1]
    t_state = snapshot(target, MAXT)
    same_state(t_state, after_forward(eng, target, trio["start"][target], fed), f"{draft} k {k}: target", slice(0, 1))
    same_state(t_state, trio["start"][target], f"{draft} k {k}: target slots 1 .. 33", slice(1, None))
    if dm is not None:
        d_state = snapshot(dm, MAXT)
        want = after_forward(eng, dm, trio["start"][dm], fed)
        draft_close(d_state, want, f"{draft} k {k}: draft state")
    # a second call continues
    restore(target, t_state)
    if dm is not None:
        restore(dm, d_state)
    more, _ = run(ids[N - 1], 8, [first] + ids[:N - 1])
    assert more.tolist() == ids[N:N + 8], draft
    # nothing is emitted or consumed beyond n_tokens
    for n in (1, k):
        reset()
        got, stats = run(first, n, [])
        assert got.tolist() == ids[:n]
        t_got, d_got = snapshot(target, MAXT), snapshot(dm, MAXT) if dm is not None else None
        same_state(t_got, after_forward(eng, target, trio["start"][target], [first] + ids[:n - 1]) if n >= 2 else t1_state(target, trio, first),
                   f"{draft} k {k} n_tokens {n}", slice(0, 1))
        if dm is not None:                                           # the draft context has consumed the same ids and no more
            restore(dm, trio["start"][dm])
            if n >= 2:
                dm.forward([first] + ids[:n - 1], eng.MODE_GPT)
            else:
                dm.forward(first)
            draft_close(d_got, snapshot(dm, MAXT), f"{draft} k {k} n_tokens {n}: draft state")


def draft_close(got, want, what):
    """slot 0 of the draft context within 1e-4, as tests/test_widths_gpu.py holds the decode kernels to the chunk path (pp: where the chunk path,
    which does not use it, was the reference, only the other four)"""
    for name, g_, r_ in zip(NAMES, got, want):
        g0, r0 = g_.view(np.float64)[0], r_.view(np.float64)[0]
        if name != "pp":
            assert np.abs(g0 - r0).max() <= 1e-4 * max(1.0, np.abs(r0).max()), f"{what} {name}"


def test_lookup_drafts_are_verified_like_any_other(eng, trio):
    """RWKV.decode_lookup with a history that DOES repeat: planted in front of the id to feed are the bigram (P, first) followed by two right ids
    and a wrong one, and a bigram of the continuation followed by four right ids -- so one draft is accepted in part, one whole, the rest of the
    rounds have nothing to guess, and the ids are still those of repeated spec_verify(n_draft = 0)"""
    target, ids, first = trio["target"], trio["ids"], trio["first"]
    P, N = 3, 24
    assert P not in ids[:N] and len(set(ids[:N])) == N and first not in ids[:N]
    fake = [P, first, ids[0], ids[1], sc.wrong(ids[2]), 7, ids[5], ids[6], ids[7], ids[8], ids[9], ids[10], 8, P]
    restore(target, trio["start"][target])
    got, stats = target.decode_lookup(fake + [first], N, k=4, n=2)
    print(f"lookup on a repeating history: rounds {stats['rounds']} drafted {stats['drafted']} accepted {stats['accepted']}")
    assert got.tolist() == ids[:N]
    assert stats == dict(rounds=N - 6, drafted=8, accepted=6), stats      # [r, r, w, 7] -> 2 stand; [r, r, r, r] -> 4 stand
    same_state(snapshot(target, MAXT), after_forward(eng, target, trio["start"][target], [first] + ids[:N - 1]), "lookup, repeating history", slice(0, 1))
    # the clamp of the draft to what n_tokens leaves room for: two ids asked, one drafted, it stands, nothing beyond is consumed
    restore(target, trio["start"][target])
    got, stats = target.decode_lookup(fake + [first], 2, k=4, n=2)
    assert got.tolist() == ids[:2] and stats == dict(rounds=1, drafted=1, accepted=1), stats
    same_state(snapshot(target, MAXT), after_forward(eng, target, trio["start"][target], [first, ids[0]]), "lookup, n_tokens 2", slice(0, 1))


def t1_state(target, trio, first):
    restore(target, trio["start"][target])
    target.spec_verify(first, [])
    return snapshot(target, MAXT)


def test_ids_equal_plain_greedy_decode_where_the_margin_is_proved(eng):
    """the model, prompt and first token of spec_cases.PLAIN: tests/test_spec_cpu.py proves on the oracle that every step's top-two gap is at
    least 1e-3 of the row's largest |logit|, 30 times what the decode kernels and the chunk path are allowed to differ by"""
    p = sc.PLAIN
    target, dm = load(eng, p["L"], p["D"], p["seed"], MAXT), load(eng, p["L"], p["D"], p["seed"], MAXT)
    for m in (target, dm):
        m.forward(list(p["prompt"]), eng.MODE_GPT)
    st = snapshot(target, MAXT)
    want = target.decode_greedy(p["first"], p["n"]).tolist()
    restore(target, st)
    got, stats = target.decode_speculative(dm, p["first"], p["n"], 4)
    assert got.tolist() == want
    restore(target, st)
    got, _ = target.decode_lookup([p["first"]], p["n"], k=8, n=2)
    assert got.tolist() == want
    target.close(); dm.close()


def test_refused_calls_leave_state_and_logits_as_they_were(eng, widths):
    L, D = sc.WIDTHS[0]
    w = widths(L, D)
    m, lib = w.m, eng.lib()
    u64 = C.c_uint64
    arr = lambda *v: (u64 * len(v))(*v)
    t = mf.synthetic_tensors(2, 64, seed=1)
    ctx = dict(M=m, U=eng.RWKV(resident=True), S=eng.RWKV(resident=True), N=eng.RWKV(resident=True), D=load(eng, 2, 64, 1, MAXT, t), D4=eng.RWKV(resident=True))
    ctx["S"].set_layer_range(0, 1)
    ctx["S"].loadTensors(2, 64, t, maxGPT=MAXT)
    ctx["N"].loadTensors(2, 64, t, maxGPT=1)                          # no chunk path: max context 1
    ctx["D4"].loadTensors(2, 64, t, maxGPT=4)
    h = {k: v._h for k, v in ctx.items()}
    out, nx = (u64 * 64)(), (u64 * 1)()
    ok, bad, long_ = arr(5, 6), arr(5, V), arr(*[5] * 40)
    cases = [
        ("rwkv_spec_verify", ("M", 5, ok, 2, None, nx), E_ARG, "NULL"),
        ("rwkv_spec_verify", ("M", 5, ok, 2, out, None), E_ARG, "NULL"),
        ("rwkv_spec_verify", ("M", 5, None, 2, out, nx), E_ARG, "NULL"),
        ("rwkv_spec_verify", ("M", 5, long_, 32, out, nx), E_ARG, "n_draft must be in 0..31"),
        ("rwkv_spec_verify", ("D4", 5, long_, 4, out, nx), E_ARG, "n_draft must be in 0..3"),
        ("rwkv_spec_verify", ("M", V, ok, 2, out, nx), E_ARG, f"token id {V} out of range"),
        ("rwkv_spec_verify", ("M", 5, bad, 2, out, nx), E_ARG, f"draft id {V} out of range"),
        ("rwkv_spec_verify", ("U", 5, ok, 2, out, nx), E_STATE, "RWKV not loaded"),
        ("rwkv_spec_verify", ("S", 5, ok, 2, out, nx), E_STATE, "whole-model"),
        ("rwkv_spec_verify", ("N", 5, ok, 0, out, nx), E_STATE, "chunked path not available"),
        ("rwkv_decode_speculative", ("M", "D", 5, 8, 0, out, None), E_ARG, "k must be in 1..31"),
        ("rwkv_decode_speculative", ("M", "D", 5, 8, 32, out, None), E_ARG, "k must be in 1..31"),
        ("rwkv_decode_speculative", ("M", "M", 5, 8, 4, out, None), E_ARG, "another context"),
        ("rwkv_decode_speculative", ("M", None, 5, 8, 4, out, None), E_ARG, "NULL"),
        ("rwkv_decode_speculative", ("M", "D", 5, 8, 4, None, None), E_ARG, "NULL"),
        ("rwkv_decode_speculative", ("M", "D4", 5, 8, 3, out, None), E_ARG, "max context >= k + 2 = 5"),
        ("rwkv_decode_speculative", ("M", "D", V, 8, 4, out, None), E_ARG, f"token id {V} out of range"),
        ("rwkv_decode_speculative", ("M", "D", 5, 0, 4, out, None), E_ARG, "n_tokens must be in 1..65536"),
        ("rwkv_decode_speculative", ("M", "U", 5, 8, 4, out, None), E_STATE, "RWKV not loaded"),
        ("rwkv_decode_speculative", ("M", "S", 5, 8, 4, out, None), E_STATE, "whole-model"),
        ("rwkv_decode_speculative", ("S", "D", 5, 8, 4, out, None), E_STATE, "whole-model"),
        ("rwkv_decode_speculative", ("N", "D", 5, 8, 4, out, None), E_STATE, "chunked path not available"),
    ]
    restore(m, w.start)
    m.forward([TOKEN] + w.g[:3], eng.MODE_GPT)                       # four logits rows and a state to keep
    state, logits = snapshot(m, MAXT), rows(m, MAXT)
    dstate = snapshot(ctx["D"], MAXT)
    for entry, args, status, text in cases:
        rc = int(getattr(lib, entry)(*[h[v] if isinstance(v, str) else v for v in args]))
        err = lib.rwkv_last_error().decode()
        print(f"{entry}{args[:1]}: status {rc}, {err!r}")
        assert rc == status and text in err, (entry, args, err)
        same_state(snapshot(m, MAXT), state, entry)
        assert np.array_equal(rows(m, MAXT), logits), entry
        same_state(snapshot(ctx["D"], MAXT), dstate, entry + " (draft)")
    for k, v in ctx.items():
        if k != "M":
            v.close()


def test_spec_app_prints_the_engine_ids(eng, tmp_path):
    L, D, n, k = 3, 64, 20, 4
    tt, td = mf.synthetic_tensors(L, D, seed=sc.SEED + 5), mf.synthetic_tensors(2, 64, seed=sc.SEED + 6)
    pt, pd = str(tmp_path / "target.bin"), str(tmp_path / "draft.bin")
    mf.write_bin(pt, L, D, tt); mf.write_bin(pd, 2, 64, td)
    target, dm = eng.RWKV(resident=True), eng.RWKV(resident=True)
    target.loadTensors(L, D, tt, maxGPT=k + 2); dm.loadTensors(2, 64, td, maxGPT=k + 2)
    app = build_app("spec_app", tmp_path)
    r = subprocess.run([app, pt, pd, str(n), str(k)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("spec_ok"), (r.returncode, r.stdout, r.stderr)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("ids", "stats", "verify", "spec_ok"))]
    assert [l.split()[0] for l in lines] == ["ids", "stats", "verify", "spec_ok"], r.stdout
    app_ids = [int(v) for v in lines[0].split()[1:]]
    for m in (target, dm):
        m.forward([5, 6, 7], eng.MODE_GPT)
    got, stats = target.decode_speculative(dm, 100, n, k)
    assert app_ids == got.tolist()
    assert lines[1] == f"stats {stats['rounds']} {stats['drafted']} {stats['accepted']}"
    target.close(); dm.close()
