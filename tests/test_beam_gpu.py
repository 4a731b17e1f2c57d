"""Beam search on the device (csrc/beam.hip.h: k_beam_select, k_beam_gather; rwkv_decode_beam / rwkv_state_permute / rwkv_debug_beam_step).
Planted steps (tests/beam_cases.py) against the brute-force np.longdouble reference: parents, tokens and ended flags equal, |d score| <= 1e-10 +
2 ulp, every token log-prob bitwise that of rwkv_score_rows, and parents, tokens and scores bitwise the host twin's on the device's own top-n.  The
state gather on distinct planted state, bitwise, at three widths and every kind of map.  The loop against the caller's loop it stands for --
copy_state forks, then per step forward(PARRALEL), topn_rows(W + 1), the host twin, a permutation through pull_state / push_state -- bitwise;
a stop id; rejected calls; buffer accounting; the C++ and pybind bindings.  Every context is a synthetic 2-layer model.
Each planted case prints its worst figure before anything is asserted."""
import ctypes as C

import numpy as np
import pytest

import beam_cases as bc
import logprob_cases as lc
import support
from support import E_ARG, E_STATE, V, build_app, eng, load, restore, run_app, rwkv_mod, same_bits, start_state  # noqa: F401

from rwkv_cpp_accelerated_amd import modelfile as mf

pytestmark = pytest.mark.gpu

L = 2
ROWS = 16                        # maxGPT of the planted context: W = 16 needs 16 rows (rows 0 .. 3 start at the four offsets from a 16-byte boundary)
D_LOOP, MAXN, STEPS = 128, 8, 12
NINF = -np.inf


def plant_state(m, seed):
    """distinct values in every element of every slot of the five arrays; returns them as [5][max_ctx][L D]"""
    rng = np.random.default_rng(seed)
    for a in m.state.arrays():
        a[:] = rng.standard_normal(a.size)
    m.push_state()
    return slots_of(m)


def slots_of(m, pull=False):
    if pull:
        m.pull_state()
    return [a.reshape(m.maxContext, -1).copy() for a in m.state.arrays()]


def check_gather(m, old, parents, logits=None):
    """slot i < n holds what slot parents[i] held, every other slot what it held; the logits are untouched"""
    new, n = slots_of(m, pull=True), len(parents)
    for a, b in zip(new, old):
        assert same_bits(a[:n], b[np.asarray(parents, np.int64)]), parents
        assert same_bits(a[n:], b[n:]), parents
    if logits is not None:
        assert same_bits(m.logits(m.maxContext), logits)


# ---- planted select -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted(eng):
    m = load(eng, L, 64, 3, ROWS)
    m.forward(5)
    yield m
    m.close()


def plant(m, rows):
    """rows: the case names of rows 0 .. W - 1"""
    support.plant_rows(m, {r: lc.logits_of(name) for r, name in enumerate(rows)}, ROWS)


@pytest.mark.parametrize("name,r", bc.case_shifts())
def test_planted_step_against_the_reference_the_scorer_and_the_host_twin(planted, rwkv_mod, name, r):
    m = planted
    rows, cum, ended, last, stops = bc.shifted(name, r)
    W = len(rows)
    plant(m, rows)
    before = m.logits(ROWS).copy()
    old = plant_state(m, 11)
    got = m.debug_beam_step(cum, ended, last, stops)
    parent, token, score, lp, end = got
    assert parent.max() < W and token.max() < V and token.min() >= 0
    want = bc.reference(name, r)
    worst, bad = bc.check(f"{name} shift {r}", got, want)
    print(f"{name:>14} shift {r}: worst |d score| {worst:.2e}  parents {parent.tolist()}  tokens {token.tolist()}")
    # every token log-prob is the scorer's, bit for bit (an ended parent's: 0.0); the score of a live parent is ONE f64 add
    s_lp, _, _ = m.score_rows(parent.tolist(), token.tolist())
    was_ended = np.array([ended[p] for p in parent.tolist()], bool)
    if not same_bits(lp, np.where(was_ended, 0.0, s_lp)):
        bad.append(f"{name}: token log-probs are not the bits of score_rows")
    if not same_bits(score, np.where(was_ended, np.array(cum)[parent], np.array(cum)[parent] + s_lp)):
        bad.append(f"{name}: scores are not cum + the scorer's log-prob")
    # parents, tokens and scores are the host twin's on the device's own top-n
    t_ids, t_lp = m.topn_rows(list(range(W)), W + 1)
    twin = rwkv_mod.beamSelect(t_ids, t_lp, np.array(cum, np.float64), list(ended), list(last), list(stops))
    if not (np.array_equal(twin[0], parent) and np.array_equal(twin[1], token) and same_bits(np.asarray(twin[2]), score)
            and same_bits(np.asarray(twin[3]), lp) and np.array_equal(twin[4], end)):
        bad.append(f"{name}: the host twin on the device's top-n gives {[np.asarray(t).tolist() for t in twin]}")
    assert not bad, bad
    check_gather(m, old, parent.tolist(), before)                                        # the step's gather; slots >= W and the logits stay


# ---- the gather ----------------------------------------------------------------------------------------------------------------
MAPS = dict(identity=list(range(8)), swap=[1, 0, 2, 3, 4, 5, 6, 7], cycle3=[0, 1, 3, 4, 2, 5, 6, 7], rotation=[1, 2, 3, 4, 5, 6, 7, 0],
            fan_out=[7] * 8, short_rotation=[4, 0, 1, 2, 3], short_fan=[2, 2, 2], one=[0], mixed=[3, 3, 0, 1, 6, 6, 4, 7])


@pytest.mark.parametrize("D", [64, 80, 128])
def test_state_permute_moves_every_slot_at_once(eng, D):
    m = load(eng, L, D, 21, 8)
    m.forward([5, 6, 7] if D != 80 else 5, eng.MODE_GPT)
    logits = m.logits(8).copy()
    for k, (name, parents) in enumerate(MAPS.items()):
        old = plant_state(m, 100 + k)
        m.state_permute(parents)
        check_gather(m, old, parents, logits)
    # the same after a selection: whatever map the step chose
    m.forward([5, 40000, 77, 9, 1234], eng.MODE_PARRALEL)
    logits = m.logits(8).copy()
    old = plant_state(m, 7)
    parent = m.debug_beam_step([-50.0, -1.0, -30.0, -20.0, -40.0], [0] * 5, [1, 2, 3, 4, 5])[0]
    assert parent[0] == 1                                                                # (the best token of any row is above -log V = -10.83)
    check_gather(m, old, parent.tolist(), logits)
    m.close()


# ---- the loop against the caller's loop it stands for --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(eng):
    m = load(eng, L, D_LOOP, 41, MAXN, head_scale=30.0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def start(eng, model):
    """distinct state in every slot: where every run of the loop tests starts"""
    return start_state(eng, model, MAXN)


def callers_loop(eng, rwkv_mod, m, first, steps, W, stops):
    """what a caller does today: fork slot 0, then per step one PARRALEL forward, topn_rows(W + 1), the selection on the host and a permutation of
    the W state slots through the host; backtracked at the end"""
    n = m.num_layers * m.num_embed
    for s in range(1, W):
        m.copy_state(s, 0)
    fed, cum, ended, ln = [int(first)] * W, np.array([0.0] + [NINF] * (W - 1)), [0] * W, [0] * W
    rec, ever = [], False
    for k in range(steps):
        m.forward(fed, eng.MODE_PARRALEL)
        ids, lp = m.topn_rows(list(range(W)), W + 1)
        parent, token, score, tlp, end = rwkv_mod.beamSelect(ids, lp, cum, ended, fed, list(stops))
        m.pull_state(W)
        for a in m.state.arrays():
            a[: W * n] = a[: W * n].reshape(W, n)[parent].reshape(-1)
        m.push_state(W)
        ln = [ln[p] if ended[p] else k + 1 for p in parent.tolist()]
        fed, cum, ended = token.tolist(), np.asarray(score, np.float64), end.tolist()
        rec.append((parent, token, np.asarray(tlp)))
        ever = ever or any(ended)
    tokens, tlps = np.zeros((W, steps), np.int64), np.zeros((W, steps))
    for h in range(W):
        at = h
        for k in range(steps - 1, -1, -1):
            if k < ln[h]:
                tokens[h, k], tlps[h, k] = rec[k][1][at], rec[k][2][at]
            at = int(rec[k][0][at])
    return tokens, np.array(ln, np.int64), cum, tlps, ended, ever


def run_both(eng, rwkv_mod, m, start, W, stops=()):
    first = 321
    restore(m, start)
    got = m.decode_beam(first, STEPS, W, stops)
    got_state = slots_of(m, pull=True)
    restore(m, start)
    want = callers_loop(eng, rwkv_mod, m, first, STEPS, W, stops)
    want_state = slots_of(m, pull=True)
    tokens, ln, score, tlp = got
    assert np.array_equal(tokens, want[0]) and np.array_equal(ln, want[1]), (tokens, want[0], ln, want[1])
    assert same_bits(score, want[2]) and same_bits(tlp, want[3])
    live = [h for h in range(W) if not want[4][h]]
    for a, b, s in zip(got_state, want_state, start):
        assert same_bits(a[live], b[live])                                               # a live hypothesis's slot: every token but the last fed
        assert same_bits(a[W:], s.view(np.float64)[W:])                                 # a call of width W leaves slots >= W alone
    for h in range(W):
        assert not tokens[h, ln[h]:].any() and not tlp[h, ln[h]:].any() and (tokens[h, : ln[h]] > 0).all()
        run = 0.0
        for v in tlp[h, : ln[h]]:
            run = run + v
        assert same_bits(np.float64(run), score[h])                                      # the score is the running sum, an ended beam keeps it
    assert np.all(np.diff(score) <= 0) and np.isfinite(score).all()                      # hypothesis 0 is the best
    return got, want[4], want[5]


@pytest.mark.parametrize("W", [2, 5, 8])
def test_the_loop_is_the_callers_loop(eng, rwkv_mod, model, start, W):
    (tokens, ln, score, tlp), ended, _ = run_both(eng, rwkv_mod, model, start, W)
    print(f"W {W}: scores {score.tolist()}\n best {tokens[0].tolist()}")
    assert ln.tolist() == [STEPS] * W and not any(ended)
    assert len({tuple(t) for t in tokens.tolist()}) == W                                 # W distinct hypotheses


@pytest.mark.parametrize("W", [2, 5, 8])
def test_a_stop_id_ends_a_beam_that_competes_on(eng, rwkv_mod, model, start, W):
    restore(model, start)
    plain = model.decode_beam(321, STEPS, W)
    stop = int(plain[0][0][3])                                                           # step 3 of the best hypothesis without stops
    (tokens, ln, score, tlp), ended, ever = run_both(eng, rwkv_mod, model, start, W, [stop])
    print(f"W {W}: stop {stop} len {ln.tolist()} ended {list(ended)} scores {score.tolist()}")
    assert ever                                                                          # a beam ended by step 3 (whether it survives is the search's business)
    for h in range(W):
        assert bool(ended[h]) == (tokens[h, ln[h] - 1] == stop)
        assert stop not in tokens[h, : ln[h] - 1].tolist()
        assert ended[h] or ln[h] == STEPS


# ---- rejected calls -----------------------------------------------------------------------------------------------------------
def test_rejected_calls_leave_everything_alone(eng, model, start):
    lib, m = eng.lib(), model
    u64, u32, dbl, u8 = C.c_uint64, C.c_uint32, C.c_double, C.c_uint8
    restore(m, start)
    m.decode_beam(5, 4, 3, [7])
    m.state_permute([1, 0])
    state, logits, resident = slots_of(m, pull=True), m.logits(MAXN).copy(), m.resident_bytes()
    tok, ln, sc_, lp = (u64 * 2048)(), (u32 * 32)(), (dbl * 32)(), (dbl * 2048)()
    stops = (u64 * 17)(*range(1, 18))

    def beam(h=m._h, first=5, steps=4, width=3, n_stop=1, stop_ids=stops, reserved=0, tokens=tok, length=ln, score=sc_, tlp=lp, null_bp=False, null_out=False):
        bp = eng.BeamParams(width, n_stop, stop_ids, reserved)
        out = eng.BeamOut(tokens, length, score, tlp)
        return int(lib.rwkv_decode_beam(h, first, steps, None if null_bp else C.byref(bp), None if null_out else C.byref(out)))

    assert beam(null_bp=True) == E_ARG and beam(null_out=True) == E_ARG
    assert beam(tokens=None) == E_ARG and beam(length=None) == E_ARG and beam(score=None) == E_ARG
    assert beam(width=0) == E_ARG and beam(width=1) == E_ARG and beam(width=17) == E_ARG and beam(width=MAXN + 1) == E_ARG
    assert beam(steps=0) == E_ARG and beam(steps=65537) == E_ARG
    assert beam(first=V) == E_ARG
    assert beam(stop_ids=(u64 * 1)(V)) == E_ARG and beam(stop_ids=(u64 * 1)(0)) == E_ARG
    assert beam(n_stop=17) == E_ARG and beam(n_stop=1, stop_ids=None) == E_ARG
    assert beam(reserved=1) == E_ARG
    par = lambda *v: (u32 * len(v))(*v)
    P = lambda p, n, h=m._h: int(lib.rwkv_state_permute(h, p, n))
    assert P(None, 2) == E_ARG and P(par(0, 1), 0) == E_ARG and P(par(*range(MAXN + 1)), MAXN + 1) == E_ARG
    assert P(par(0, 2), 2) == E_ARG and P(par(3, 0, 1), 3) == E_ARG
    cum, end, last = (dbl * 16)(), (u8 * 16)(), (u64 * 16)(*range(1, 17))
    o_par, o_tok, o_sc, o_lp, o_end = (u32 * 16)(), (u64 * 16)(), (dbl * 16)(), (dbl * 16)(), (u8 * 16)()

    def step(h=m._h, width=3, n_stop=0, stop_ids=None, reserved=0, cum=cum, end=end, last=last, o_par=o_par, o_tok=o_tok, o_sc=o_sc, o_lp=o_lp, o_end=o_end, null_bp=False):
        bp = eng.BeamParams(width, n_stop, stop_ids, reserved)
        return int(lib.rwkv_debug_beam_step(h, None if null_bp else C.byref(bp), cum, end, last, o_par, o_tok, o_sc, o_lp, o_end))

    assert step(null_bp=True) == E_ARG and step(cum=None) == E_ARG and step(end=None) == E_ARG and step(last=None) == E_ARG
    assert step(o_par=None) == E_ARG and step(o_tok=None) == E_ARG and step(o_sc=None) == E_ARG and step(o_lp=None) == E_ARG and step(o_end=None) == E_ARG
    assert step(width=1) == E_ARG and step(width=17) == E_ARG and step(width=MAXN + 1) == E_ARG
    assert step(last=(u64 * 3)(1, V, 2)) == E_ARG and step(n_stop=1, stop_ids=(u64 * 1)(0)) == E_ARG and step(n_stop=17, stop_ids=stops) == E_ARG
    assert step(n_stop=1) == E_ARG and step(reserved=5) == E_ARG
    for x, y in zip(state, slots_of(m, pull=True)):
        assert same_bits(x, y)
    assert same_bits(logits, m.logits(MAXN)) and m.resident_bytes() == resident
    # accepted: no stop ids, no token log-probs
    assert beam(n_stop=0, stop_ids=None, tlp=None) == 0 and P(par(0, 1), 2) == 0 and step() == 0
    # not loaded
    e = eng.RWKV(resident=True)
    assert beam(h=e._h) == E_STATE and P(par(0, 1), 2, h=e._h) == E_STATE and step(h=e._h) == E_STATE
    assert beam(h=e._h, null_bp=True) == E_ARG and P(None, 2, h=e._h) == E_ARG
    e.close()
    # pipeline stages: no stage searches; the gather needs only a loaded context
    t = mf.synthetic_tensors(L, 64, seed=3)
    for (l0, l1) in ((0, 1), (1, 2)):
        e = eng.RWKV(resident=True)
        e.set_layer_range(l0, l1)
        e.loadTensors(L, 64, t, maxGPT=4)
        assert beam(h=e._h) == E_STATE and step(h=e._h) == E_STATE
        old = plant_state(e, 3)
        e.state_permute([2, 0, 1])
        check_gather(e, old, [2, 0, 1])
        e.close()
    # a context without the chunk path does not search
    e = load(eng, L, 48, 42, 4)
    assert beam(h=e._h) == E_STATE
    e.close()


# ---- buffer accounting --------------------------------------------------------------------------------------------------------
def beam_bytes(W, steps, D):
    """include/rwkv_mi355x.h: the record 8 (5 W + 16 + 3 W n_steps), the staging buffer 40 W L D, and the top-n scratch of the log-prob block for W
    rows, one step and n = W + 1 (tests/test_logprobs_gpu.py record_bytes)"""
    topn = W * (8 + 128 * (4 + W + 1)) + W * 16 * (1 + W + 1)
    return 8 * (5 * W + 16 + 3 * W * steps), 40 * W * L * D, topn


def test_the_buffers_are_counted(eng):
    D = 64
    m = load(eng, L, D, 9, 8)
    m.forward([5, 6, 7, 8, 9, 10, 11, 12], eng.MODE_PARRALEL)
    base = m.resident_bytes()
    m.decode_beam(5, 6, 4)
    assert m.resident_bytes() - base == sum(beam_bytes(4, 6, D))
    r1 = m.resident_bytes()
    m.decode_beam(5, 5, 3, [9])
    m.state_permute([1, 0, 2, 3])
    m.debug_beam_step([0.0, -1.0], [0, 0], [1, 2])
    assert m.resident_bytes() == r1                                          # smaller calls fit
    m.state_permute(list(range(1, 8)) + [0])
    assert m.resident_bytes() - r1 == 40 * 8 * L * D - 40 * 4 * L * D        # the staging buffer alone grows
    r2 = m.resident_bytes()
    m.decode_beam(5, 9, 4)
    assert m.resident_bytes() - r2 == beam_bytes(4, 9, D)[0] - beam_bytes(4, 6, D)[0]
    m.close()
    m = load(eng, L, D, 9, 8)                                                # the gather alone: the map and the staging buffer
    base = m.resident_bytes()
    m.state_permute([2, 0, 1])
    assert m.resident_bytes() - base == 8 * 2 + 40 * 3 * L * D
    m.close()


# ---- bindings -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_file(tmp_path_factory):
    return support.model_file(tmp_path_factory, "beam", L, D_LOOP, 43, head_scale=30.0)


def test_beam_app_matches_the_python_engine(eng, built, model_file, tmp_path):
    W, steps = 4, 7
    m = eng.RWKV(resident=True)
    m.loadFile(model_file, W + 1)
    m.forward([5, 6, 7], eng.MODE_GPT)
    plain = m.decode_beam(100, steps, W)
    stop = int(plain[0][0][2])
    m.reset_state()
    m.forward([5, 6, 7], eng.MODE_GPT)
    tokens, ln, score, tlp = m.decode_beam(100, steps, W, [stop])
    m.close()
    rc, lines, raw = run_app(build_app("beam_app", tmp_path), [model_file, W, steps, stop])
    assert rc == 0, raw
    lines = [l.split() for l in lines]
    assert lines[-1] == ["beam_ok"] and len(lines) == W + 1
    hx = float.fromhex
    for f in lines[:W]:
        h = int(f[0])
        assert int(f[1]) == ln[h] and hx(f[2]).hex() == float(score[h]).hex(), h
        assert [int(v) for v in f[3::2]] == tokens[h].tolist() and [hx(v).hex() for v in f[4::2]] == [float(v).hex() for v in tlp[h]], h


def test_pybind_decode_beam_matches_the_python_engine(eng, rwkv_mod, model_file):
    W, steps = 3, 6
    h = rwkv_mod.initRwkv()
    rwkv_mod.loadModel(h, model_file, W)
    rwkv_mod.initOutput(h); rwkv_mod.initState(h)
    rwkv_mod.modelForward(h, 1234)
    got = rwkv_mod.decodeBeam(h, 77, steps, W, [])
    rwkv_mod.freeRwkv(h)
    m = eng.RWKV(resident=True)
    m.loadFile(model_file, W)
    m.forward(1234)
    tokens, ln, score, tlp = m.decode_beam(77, steps, W)
    m.close()
    assert got[0].shape == (W, steps) and np.array_equal(got[0], tokens) and np.array_equal(got[1], ln)
    assert same_bits(np.asarray(got[2]), score) and same_bits(np.asarray(got[3]), tlp)
