"""Device-side batched decode (rwkv_decode_batch_greedy / rwkv_decode_batch_typical / rwkv_state_copy): N streams on state
slots 0 .. N - 1, every step the rwkv_forward(N, PARRALEL) schedule with the ids fed from the device and the pick over all
rows on the device.  Checked against the host loop over the same engine (bit for bit: same kernels), the CPU oracle,
the single-stream decode loops, and for its argument checks."""
import ctypes as C
import os

import numpy as np
import pytest

from rwkv_cpp_accelerated_amd import modelfile as mf
import parity
from sampler_cases import splitmix_u
from support import E_ARG, E_STATE, eng, load, restore, snapshot, start_state  # noqa: F401

pytestmark = pytest.mark.gpu

L, D, MAXN = 3, 256, 96          # three layers: a call of more than 64 rows runs the three-stage pipeline


@pytest.fixture(scope="module")
def tensors():
    return mf.synthetic_tensors(L, D, seed=21, head_scale=30.0)


@pytest.fixture(scope="module")
def model(eng, tensors):
    m = load(eng, L, D, 21, MAXN, tensors)
    yield m
    m.close()


def host_greedy(eng, m, first, n_steps):
    ids, out = list(first), []
    for _ in range(n_steps):
        lg = m.forward(ids, eng.MODE_PARRALEL)[: len(ids) * mf.VOCAB].reshape(len(ids), mf.VOCAB)
        ids = [parity.argmax_ban0(lg[s]) for s in range(len(ids))]
        out.append(ids)
    return np.array(out, np.int64).T


def host_typical(eng, m, first, n_steps, seeds, temp, tau, recipe):
    ids, out = list(first), []
    for k in range(n_steps):
        m.forward(ids, eng.MODE_PARRALEL)
        ids = [m.sample_typical(temp, tau, splitmix_u(seeds[s], k), row=s, ban0=True, recipe=recipe) for s in range(len(ids))]
        out.append(ids)
    return np.array(out, np.int64).T


def first_tokens(n, seed=3):
    return [int(v) for v in np.random.default_rng(seed).integers(1, mf.VOCAB, n)]


@pytest.mark.parametrize("n", [2, 32, 64, 96])
def test_greedy_equals_host_loop_bit_for_bit(eng, model, n):
    m, steps = model, 6
    snap = start_state(eng, m, MAXN)
    first = first_tokens(n)
    got = m.decode_batch_greedy(first, steps).astype(np.int64)
    dev_state = snapshot(m, n)
    dev_logits = m.logits(n).copy()
    restore(m, snap)
    want = host_greedy(eng, m, first, steps)
    assert got.shape == (n, steps)
    assert np.array_equal(got, want)
    for a, b in zip(dev_state, snapshot(m, n)):
        assert np.array_equal(a, b)                       # bit-equal state of all N slots
    assert np.array_equal(dev_logits, m.logits(n))        # the last step's logits stay in rows 0 .. N - 1


@pytest.mark.parametrize("recipe", [False, True])
def test_typical_equals_host_loop(eng, model, recipe):
    m, n, steps, temp, tau = model, 40, 5, 0.45, 0.8
    snap = start_state(eng, m, MAXN)
    first, seeds = first_tokens(n, 4), [1000 + 7 * s for s in range(n)]
    got = m.decode_batch_typical(first, steps, temp=temp, tau=tau, seeds=seeds, recipe=recipe).astype(np.int64)
    dev_state = snapshot(m, n)
    restore(m, snap)
    want = host_typical(eng, m, first, steps, seeds, temp, tau, recipe)
    assert np.array_equal(got, want)
    for a, b in zip(dev_state, snapshot(m, n)):
        assert np.array_equal(a, b)


def test_streams_are_isolated(eng, model):
    m, steps = model, 5
    snap = start_state(eng, m, MAXN)
    first, seeds = first_tokens(8, 6), list(range(50, 58))
    g8 = m.decode_batch_greedy(first, steps); restore(m, snap)
    g4 = m.decode_batch_greedy(first[:4], steps); restore(m, snap)
    assert np.array_equal(g8[:4], g4)
    t8 = m.decode_batch_typical(first, steps, seeds=seeds); restore(m, snap)
    t4 = m.decode_batch_typical(first[:4], steps, seeds=seeds[:4]); restore(m, snap)
    assert np.array_equal(t8[:4], t4)
    f2 = list(first); f2[5] = (f2[5] + 1234) % mf.VOCAB or 1
    g8b = m.decode_batch_greedy(f2, steps); restore(m, snap)
    keep = [s for s in range(8) if s != 5]
    assert np.array_equal(g8[keep], g8b[keep]) and not np.array_equal(g8[5], g8b[5])
    s2 = list(seeds); s2[5] = 999
    t8b = m.decode_batch_typical(first, steps, seeds=s2); restore(m, snap)
    assert np.array_equal(t8[keep], t8b[keep])


def test_greedy_agrees_with_the_oracle(eng, model, tensors):
    import oracle_lib
    m, n, steps = model, 3, 8
    m.reset_state()
    first = [11, 4242, 30000]
    got = m.decode_batch_greedy(first, steps)
    o = oracle_lib.Oracle()
    om = o.from_tensors(L, D, tensors)
    st = om.new_state(n)
    ids = list(first)
    for k in range(steps):
        lg = om.forward(ids, st, mode=oracle_lib.MODE_PARRALEL)
        nxt = []
        for s in range(n):
            r = parity.argmax_ban0(lg[s])
            if r != int(got[s, k]):       # only inside the tolerance band: the reference's top-2 margin
                rr = np.array(lg[s], np.float64); rr[0] = -np.inf
                assert rr.max() - rr[int(got[s, k])] <= 2 * parity.REL * np.abs(rr[np.isfinite(rr)]).max(), f"stream {s} step {k}"
                r = int(got[s, k])        # follow the device past a near-tie
            nxt.append(r)
        ids = nxt
    om.close()


def test_one_stream_is_the_decode_loop(eng, model):
    m, steps = model, 12
    m.reset_state(); m.forward([5, 6, 7], eng.MODE_GPT)
    snap = snapshot(m, 1)
    got = m.decode_batch_greedy([42], steps)[0]
    restore(m, snap)
    assert np.array_equal(got, m.decode_greedy(42, steps))
    for recipe in (False, True):
        restore(m, snap)
        got = m.decode_batch_typical([42], steps, temp=0.45, seeds=[77], recipe=recipe)[0]
        restore(m, snap)
        assert np.array_equal(got, m.decode_typical(42, steps, temp=0.45, seed=77, recipe=recipe))


def test_fork_a_prompt_into_slots(eng, model):
    m, n, steps = model, 8, 10
    m.reset_state()
    m.forward([3, 1000, 2000, 15, 9, 77, 40000], eng.MODE_GPT)       # prefill on slot 0
    for s in range(1, n):
        m.copy_state(s, 0)
    snap = snapshot(m, n)
    for a in snap:
        for s in range(1, n):
            assert np.array_equal(a[s], a[0])
    g = m.decode_batch_greedy([500] * n, steps)
    assert all(np.array_equal(g[s], g[0]) for s in range(n))
    restore(m, snap)
    t = m.decode_batch_typical([500] * n, steps, temp=1.0, tau=0.9, seeds=list(range(n)))
    assert not all(np.array_equal(t[s], t[0]) for s in range(n))
    restore(m, snap)
    assert np.array_equal(t, m.decode_batch_typical([500] * n, steps, temp=1.0, tau=0.9, seeds=list(range(n))))


def _status(fn, *args):
    return int(fn(*args))


def test_rejected_calls_leave_the_state_alone(eng, model, tensors):
    lib, m = eng.lib(), model
    u64 = C.c_uint64
    start_state(eng, m, 4)
    before = snapshot(m, MAXN)
    out = (u64 * 4096)()
    ft = lambda *v: (u64 * len(v))(*v)
    seeds = ft(1, 2, 3, 4)
    G = lambda first, n, steps, o=out: _status(lib.rwkv_decode_batch_greedy, m._h, first, n, steps, o)
    T = lambda first, n, steps, temp=0.9, sd=seeds, o=out: _status(lib.rwkv_decode_batch_typical, m._h, first, n, steps, temp, 0.8, sd, 0, o)
    assert G(None, 2, 4) == E_ARG
    assert G(ft(1, 2), 2, 4, None) == E_ARG
    assert T(ft(1, 2), 2, 4, sd=None) == E_ARG
    assert G(ft(1, 2), 0, 4) == E_ARG and T(ft(1, 2), 0, 4) == E_ARG
    assert G((u64 * (MAXN + 1))(*[1] * (MAXN + 1)), MAXN + 1, 1) == E_ARG
    assert G(ft(1, 2), 2, 0) == E_ARG and T(ft(1, 2), 2, 0) == E_ARG
    assert G(ft(1, 2), 2, 65537) == E_ARG
    assert G(ft(1, mf.VOCAB), 2, 4) == E_ARG and T(ft(mf.VOCAB, 1), 2, 4) == E_ARG
    for bad in (0.0, -1.0, float("nan")):
        assert T(ft(1, 2), 2, 4, temp=bad) == E_ARG
    assert _status(lib.rwkv_state_copy, m._h, MAXN, 0) == E_ARG
    assert _status(lib.rwkv_state_copy, m._h, 0, MAXN) == E_ARG
    for a, b in zip(before, snapshot(m, MAXN)):
        assert np.array_equal(a, b)
    # not loaded
    e = eng.RWKV(resident=True)
    assert _status(lib.rwkv_decode_batch_greedy, e._h, ft(1, 2), 2, 4, out) == E_STATE
    assert _status(lib.rwkv_decode_batch_typical, e._h, ft(1, 2), 2, 4, 0.9, 0.8, seeds, 0, out) == E_STATE
    assert _status(lib.rwkv_state_copy, e._h, 1, 0) == E_STATE
    e.close()
    # a pipeline stage (layers [0, 2) of 3: no head)
    e = eng.RWKV(resident=True)
    e.set_layer_range(0, 2)
    e.loadTensors(L, D, tensors, maxGPT=4)
    assert _status(lib.rwkv_decode_batch_greedy, e._h, ft(1, 2), 2, 4, out) == E_STATE
    assert _status(lib.rwkv_decode_batch_typical, e._h, ft(1), 1, 4, 0.9, 0.8, seeds, 0, out) == E_STATE
    e.close()
    # the chunk path off: one stream still runs (the decode kernels), two do not
    os.environ["RWKV_SEQ"] = "0"
    try:
        e = eng.RWKV(resident=True)
        e.loadTensors(L, D, tensors, maxGPT=4)
    finally:
        del os.environ["RWKV_SEQ"]
    e.forward([1, 2], eng.MODE_PARRALEL)
    e.pull_state(4)
    st = [a.copy() for a in e.state.arrays()]
    assert _status(lib.rwkv_decode_batch_greedy, e._h, ft(1, 2), 2, 4, out) == E_STATE
    assert _status(lib.rwkv_decode_batch_typical, e._h, ft(1, 2), 2, 4, 0.9, 0.8, seeds, 0, out) == E_STATE
    e.pull_state(4)
    for a, b in zip(st, e.state.arrays()):
        assert np.array_equal(a, b)
    assert _status(lib.rwkv_decode_batch_greedy, e._h, ft(1), 1, 4, out) == 0
    e.close()


def test_host_authoritative_mode(eng, tensors):
    m = eng.RWKV(resident=False)
    m.loadTensors(L, D, tensors, maxGPT=8)
    n = 6
    m.forward(first_tokens(n, 8), eng.MODE_PARRALEL)
    m.forward(first_tokens(n, 9), eng.MODE_PARRALEL)
    host_before = [a.copy() for a in m.state.arrays()]
    ids = m.decode_batch_greedy(first_tokens(n, 10), 5)
    dev = [np.zeros(8 * L * D) for _ in range(5)]
    assert eng.lib().rwkv_get_output(m._h, None, *[C.c_void_p(a.ctypes.data) for a in dev], 8) == 0
    k = n * L * D
    for h, d in zip(m.state.arrays(), dev):
        assert np.array_equal(h[:k], d[:k])
    assert any(not np.array_equal(h[:k], b[:k]) for h, b in zip(m.state.arrays(), host_before))   # (pp stays 0, as in the reference)
    m.decode_batch_typical(first_tokens(n, 11), 5, seeds=list(range(n)))
    assert eng.lib().rwkv_get_output(m._h, None, *[C.c_void_p(a.ctypes.data) for a in dev], 8) == 0
    for h, d in zip(m.state.arrays(), dev):
        assert np.array_equal(h[:k], d[:k])
    m.copy_state(7, 0)
    per = L * D
    for h in m.state.arrays():
        assert np.array_equal(h[7 * per:8 * per], h[:per])
    assert ids.shape == (n, 5)
    m.close()
