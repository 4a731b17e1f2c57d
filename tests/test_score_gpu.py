"""The device scorer (csrc/score.hip.h: k_score_part, k_score_finish; rwkv_score_rows / rwkv_score) against the f64 reference of
tests/score_cases.py: |d logprob| <= 1e-10, |d entropy| <= 1e-9, argmax equal, a -inf log-probability exactly -inf (where the bounds come
from: score_cases' docstring).  Planted rows at all four row alignments; rwkv_score bit-tied to a loop of rwkv_forward; rows after a
PARRALEL step; rejected calls; scratch accounting; the C++ and pybind bindings.  Every context is a synthetic 2-layer model.
Each planted case prints its worst figures before anything is asserted (the table is in profiles/NOTES.md, "scoring on the device")."""
import ctypes as C

import numpy as np
import pytest

import score_cases as sc
import support
from support import E_ARG, E_STATE, build_app, eng, load, restore, run_app, rwkv_mod, same_state, snapshot  # noqa: F401

from rwkv_cpp_accelerated_amd import modelfile as mf

pytestmark = pytest.mark.gpu

L = 2
ROWS = 4                         # maxGPT of the planted context: rows 0 .. 3 start at the four offsets from a 16-byte boundary
D_SEQ, MAX_SEQ = 128, 40         # the sequence context: a chunk path, pieces of 40 tokens
D_TOK, MAX_TOK = 48, 3           # a width without a chunk path: every piece runs token by token


@pytest.fixture(scope="module")
def planted(eng):
    m = load(eng, L, 64, 3, ROWS)
    m.forward(5)
    yield m
    m.close()


@pytest.fixture(scope="module")
def seq(eng):
    m = load(eng, L, D_SEQ, 41, MAX_SEQ, head_scale=30.0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def tok(eng):
    m = load(eng, L, D_TOK, 42, MAX_TOK, head_scale=30.0)
    yield m
    m.close()


def plant(m, rows):
    """rows: {logits row: case name}"""
    support.plant_rows(m, {r: sc.logits_of(name) for r, name in rows.items()}, ROWS)


def want_of(queries):
    """queries: (case, target) -> the reference's (logprob, entropy, argmax) arrays"""
    return (np.array([sc.ref_of(n)[0][g] for n, g in queries]), np.array([sc.ref_of(n)[1] for n, g in queries]),
            np.array([sc.ref_of(n)[2] for n, g in queries]))


# ---- planted rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.CASES)
def test_planted_case_on_each_of_the_four_row_alignments(planted, name):
    m = planted
    plant(m, {r: name for r in range(ROWS)})
    before = m.logits(ROWS).copy()
    rows = [r for r in range(ROWS) for _ in sc.targets_of(name)]
    targets = sc.targets_of(name) * ROWS
    lp, ent, am = m.score_rows(rows, targets)
    wl, we, bad = sc.check(name, lp, ent, am, *want_of([(name, g) for g in targets]))
    print(f"{name:>10}: queries {len(rows)}  worst |d logprob| {wl:.2e}  worst |d entropy| {we:.2e}  argmax {int(am[0])}  -inf targets {int(np.isneginf(lp).sum())}")
    assert not bad, bad
    assert np.array_equal(before.view(np.uint32), m.logits(ROWS).view(np.uint32))       # scoring leaves the logits alone


def test_one_call_repeats_rows_out_of_order_across_different_cases(planted):
    m = planted
    held = {0: "wide", 1: "neginf", 2: "ties", 3: "peak800"}
    plant(m, held)
    rows = [3, 0, 3, 2, 1, 1, 0, 3, 2, 0]
    targets = [25000, sc.V - 1, 0, 51, 1, 0, sc.ref_of("wide")[2], sc.V - 64, sc.V - 1, 50176]
    lp, ent, am = m.score_rows(rows, targets)
    wl, we, bad = sc.check("mixed", lp, ent, am, *want_of([(held[r], g) for r, g in zip(rows, targets)]))
    print(f"     mixed: queries {len(rows)}  worst |d logprob| {wl:.2e}  worst |d entropy| {we:.2e}")
    assert not bad, bad
    assert lp[4] == -np.inf                                                              # target 1 of `neginf`


# ---- a sequence, bit-tied to rwkv_forward -------------------------------------------------------------------------------------------
def sequence_case(eng, m, n, seed):
    rng = np.random.default_rng(seed)
    tokens = [int(v) for v in rng.integers(0, mf.VOCAB, n)]
    targets = [int(v) for v in rng.integers(0, mf.VOCAB, n)]
    m.reset_state()
    m.forward([11, 4242, 30000][: min(3, m.maxContext)], eng.MODE_GPT)                   # "from the current state": not the zero state
    start = snapshot(m, 1)
    lp, ent, am = m.score(tokens, targets)
    dev_state = snapshot(m, 1)
    last = n % m.maxContext or m.maxContext
    dev_logits = m.logits(last).copy()
    restore(m, start)
    w_lp, w_ent, w_am = [], [], []
    for t0 in range(0, n, m.maxContext):                                                # the caller's loop the call stands for
        piece = tokens[t0:t0 + m.maxContext]
        lg = m.forward(piece, eng.MODE_GPT)[: len(piece) * mf.VOCAB].reshape(len(piece), mf.VOCAB)
        for i in range(len(piece)):
            r = sc.reference(lg[i])
            w_lp.append(r[0][targets[t0 + i]]); w_ent.append(r[1]); w_am.append(r[2])
    wl, we, bad = sc.check(f"n={n}", lp, ent, am, w_lp, w_ent, w_am)
    print(f"D {m.num_embed} n {n}: worst |d logprob| {wl:.2e}  worst |d entropy| {we:.2e}")
    assert not bad, bad
    same_state(dev_state, snapshot(m, 1), f"n={n}")                                      # the final state, bit for bit
    assert np.array_equal(dev_logits.view(np.uint32), m.logits(last).view(np.uint32))   # the logits buffer holds the last piece's rows


@pytest.mark.parametrize("n", [3, 40, 81, 85])
def test_score_is_the_loop_of_forwards(eng, seq, n):
    """3: one short pass; 40: one two-half pass; 81: pieces of 40 + 40 + 1, the last through the decode kernels; 85: remainder 5"""
    sequence_case(eng, seq, n, 100 + n)


def test_score_at_a_width_without_a_chunk_path(eng, tok):
    sequence_case(eng, tok, 8, 7)                                                        # pieces of 3 + 3 + 2, token by token


def test_score_of_a_document_defaults_to_next_token_targets(eng, seq):
    doc = [3, 1000, 2000, 15, 9, 77, 40000]
    seq.reset_state()
    a = seq.score(doc)
    seq.reset_state()
    b = seq.score(doc[:-1], doc[1:])
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a[0]) == len(doc) - 1


# ---- rows after a PARRALEL step -----------------------------------------------------------------------------------------------------
def test_rows_after_a_parralel_step(eng, seq):
    m = seq
    m.reset_state()
    lg = m.forward([5, 40000, 77], eng.MODE_PARRALEL)[: 3 * mf.VOCAB].reshape(3, mf.VOCAB).copy()
    rows, targets = [2, 0, 1, 0], [9, int(np.argmax(lg[0])), sc.V - 1, 0]
    lp, ent, am = m.score_rows(rows, targets)
    refs = [sc.reference(lg[r]) for r in rows]
    wl, we, bad = sc.check("parralel", lp, ent, am, [r[0][g] for r, g in zip(refs, targets)], [r[1] for r in refs], [r[2] for r in refs])
    print(f"  parralel: worst |d logprob| {wl:.2e}  worst |d entropy| {we:.2e}")
    assert not bad, bad


# ---- rejected calls ---------------------------------------------------------------------------------------------------------------
def test_rejected_calls_leave_state_and_logits_alone(eng, seq):
    lib, m = eng.lib(), seq
    u64 = C.c_uint64
    m.reset_state()
    m.forward([5, 6, 7, 8], eng.MODE_GPT)
    state, logits = snapshot(m, 1), m.logits(MAX_SEQ).copy()
    a = lambda *v: (u64 * len(v))(*v)
    lp, ent, am = (C.c_double * 4)(), (C.c_double * 4)(), (u64 * 4)()
    R = lambda rows, targets, n, out=lp: int(lib.rwkv_score_rows(m._h, rows, targets, n, out, ent, am))
    S = lambda tokens, targets, n, out=lp: int(lib.rwkv_score(m._h, tokens, targets, n, out, ent, am))
    assert R(a(0, MAX_SEQ), a(1, 2), 2) == E_ARG                  # a row = max_ctx
    assert R(a(0, 1), a(1, mf.VOCAB), 2) == E_ARG                 # a target = 50277
    assert R(a(0, 1), a(1, 2), 0) == E_ARG                        # n = 0
    assert R(a(0, 1), a(1, 2), 65537) == E_ARG
    assert R(None, a(1, 2), 2) == E_ARG and R(a(0, 1), None, 2) == E_ARG and R(a(0, 1), a(1, 2), 2, None) == E_ARG
    assert S(a(1, 2), a(1, mf.VOCAB), 2) == E_ARG
    assert S(a(1, mf.VOCAB), a(1, 2), 2) == E_ARG                 # a token = 50277, behind a good one
    assert S(a(1, 2), a(1, 2), 0) == E_ARG and S(a(1, 2), a(1, 2), 65537) == E_ARG
    assert S(None, a(1, 2), 2) == E_ARG and S(a(1, 2), None, 2) == E_ARG and S(a(1, 2), a(1, 2), 2, None) == E_ARG
    same_state(state, snapshot(m, 1), "rejected calls")
    assert np.array_equal(logits.view(np.uint32), m.logits(MAX_SEQ).view(np.uint32))
    assert R(a(0, 1), a(1, 2), 2) == 0 and S(a(1, 2), a(1, 2), 2) == 0        # entropy and argmax may be NULL
    assert int(lib.rwkv_score_rows(m._h, a(0), a(1), 1, lp, None, None)) == 0
    # not loaded
    e = eng.RWKV(resident=True)
    assert int(lib.rwkv_score_rows(e._h, a(0), a(1), 1, lp, ent, am)) == E_STATE
    assert int(lib.rwkv_score(e._h, a(0), a(1), 1, lp, ent, am)) == E_STATE
    assert int(lib.rwkv_score_rows(e._h, None, a(1), 1, lp, ent, am)) == E_ARG
    assert int(lib.rwkv_score(e._h, a(0), a(1), 1, None, ent, am)) == E_ARG
    e.close()
    # pipeline stages: the first of two holds no head; the last one does, and scores the rows it holds (zeros: the uniform distribution)
    t = mf.synthetic_tensors(L, 64, seed=3)
    for (l0, l1, rows_status) in ((0, 1, E_STATE), (1, 2, 0)):
        e = eng.RWKV(resident=True)
        e.set_layer_range(l0, l1)
        e.loadTensors(L, 64, t, maxGPT=2)
        assert int(lib.rwkv_score_rows(e._h, a(1), a(7), 1, lp, ent, am)) == rows_status
        if rows_status == 0:
            assert abs(lp[0] + np.log(sc.V)) < 1e-10 and abs(ent[0] - np.log(sc.V)) < 1e-9 and am[0] == 0
        assert int(lib.rwkv_score(e._h, a(1), a(7), 1, lp, ent, am)) == E_STATE
        e.close()


# ---- scratch accounting -------------------------------------------------------------------------------------------------------------
def test_scratch_is_counted_once_per_size(eng):
    m = load(eng, L, 64, 9, 2)
    m.forward([5, 6], eng.MODE_GPT)
    r0 = m.resident_bytes()
    m.score_rows([0, 1, 0], [1, 2, 3])
    r1 = m.resident_bytes()
    m.score_rows([1, 1, 0], [4, 5, 6])
    assert r1 > r0 and m.resident_bytes() == r1
    m.score([1, 2, 3], [4, 5, 6])                   # (a piece of two through the chunk path and one token through the decode kernels)
    r2 = m.resident_bytes()
    m.score([7, 8, 9], [1, 2, 3])
    assert m.resident_bytes() == r2
    m.score_rows([0] * 9, [1] * 9)
    assert m.resident_bytes() > r1
    m.close()


# ---- bindings ---------------------------------------------------------------------------------------------------------------------
PROMPT = [3, 1000, 2000, 15, 9, 77, 40000, 5, 50276, 0, 31337]


@pytest.fixture(scope="module")
def model_file(tmp_path_factory):
    return support.model_file(tmp_path_factory, "score", L, D_SEQ, 43, head_scale=30.0)


def test_score_app_matches_the_python_engine(eng, built, model_file, tmp_path_factory):
    app, max_ctx = build_app("score_app", tmp_path_factory.mktemp('cpp')), 4
    rc, lines, raw = run_app(app, [model_file, max_ctx] + PROMPT)
    assert rc == 0, raw
    assert lines[-1] == "score_ok"
    n, last = len(PROMPT) - 1, (len(PROMPT) - 1) % max_ctx or max_ctx
    got = np.array([float(l) for l in lines[-1 - last - n:-1 - last]])
    got_rows = [l.split() for l in lines[-1 - last:-1]]
    m = eng.RWKV(resident=True)
    m.loadFile(model_file, max_ctx)
    lp, ent, am = m.score(PROMPT)
    assert np.array_equal(got, lp)
    rl, re, ra = m.score_rows(list(range(last)), PROMPT[:last])
    assert np.array_equal(np.array([float(r[0]) for r in got_rows]), rl) and np.array_equal(np.array([float(r[1]) for r in got_rows]), re)
    assert [int(r[2]) for r in got_rows] == ra.tolist()
    m.close()


def test_pybind_score_tokens_matches_the_python_engine(eng, rwkv_mod, model_file):
    rwkv = rwkv_mod
    h = rwkv.initRwkv()
    rwkv.loadModel(h, model_file)
    rwkv.initOutput(h); rwkv.initState(h)
    got = rwkv.scoreTokens(h, PROMPT)
    rwkv.freeRwkv(h)
    m = eng.RWKV(resident=True)
    m.loadFile(model_file)                           # maxGPT 1, as loadModel: ten pieces of one token, the decode kernels
    lp, _, _ = m.score(PROMPT)
    m.close()
    assert got.dtype == np.float64 and got.shape == (len(PROMPT) - 1,) and np.array_equal(got, lp)
    assert np.isfinite(lp).all() and (lp < 0).all()
