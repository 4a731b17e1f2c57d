"""The widths the chunk path does not take.  The loader accepts every n_embed that is a multiple of 16 up to 5120; the chunked prompt
path (mm8_seq, csrc/seq.hip.h) exists for the multiples of 64 only.  At the other widths a context loaded with max_ctx > 1 runs
rwkv_forward(T >= 2) token by token on the decode kernels, in both modes, and every entry point that needs the chunk path answers
RWKV_E_STATE before anything is launched.  D = 80: below 256, most workgroups own no channel; D = 1040: uneven shares (4 and 5 channels)
and one live lane in the second 1 KiB step of the quantised vector."""
import ctypes as C

import numpy as np
import pytest

from rwkv_cpp_accelerated_amd import modelfile as mf
import parity
from support import E_STATE, eng  # noqa: F401

pytestmark = pytest.mark.gpu
L, MAXT, T = 2, 8, 5
WIDTHS = [80, 1040]


def _toks(n, seed):
    return [int(v) for v in np.random.default_rng(seed).integers(2, mf.VOCAB, n)]


def _load(eng, D, seed):
    t = mf.synthetic_tensors(L, D, seed=seed)
    m = eng.RWKV(resident=True)
    m.loadTensors(L, D, t, maxGPT=MAXT)
    return t, m


def _snapshot(m):
    m.pull_state(MAXT)
    return [a.copy() for a in m.state.arrays()]


@pytest.mark.parametrize("mode", ["gpt", "par"])
@pytest.mark.parametrize("D", WIDTHS)
def test_forward_of_several_tokens_falls_back_to_token_by_token_and_matches_the_oracle(eng, oracle, D, mode):
    """forward(5 tokens) in GPT mode (one sequence on slot 0) and in PARRALEL mode (five sequences on slots 0 .. 4), three rounds that
    continue from each other's state: every logits row, its argmax and the five state arrays over all eight slots are the oracle's"""
    t, m = _load(eng, D, 1300 + D)
    om = oracle.from_tensors(L, D, t)
    st = om.new_state(slots=MAXT)
    md, omode = (eng.MODE_GPT, 1) if mode == "gpt" else (eng.MODE_PARRALEL, 0)
    for rnd in range(3):
        toks = _toks(T, 100 * rnd + D)
        ref = om.forward(toks, st, mode=omode)
        got = m.forward(toks, md)[: T * mf.VOCAB].reshape(T, mf.VOCAB).copy()
        for i in range(T):
            parity.check_logits(got[i], ref[i], f"D{D} {mode} round {rnd} row {i}")
            parity.check_argmax(got[i], ref[i], f"D{D} {mode} round {rnd} row {i}")
    for name, g, r in zip("xy aa bb pp dd".split(), _snapshot(m), st):
        assert np.abs(g - r).max() <= 1e-4 * max(1.0, np.abs(r).max()), name
    om.close(); m.close()


@pytest.mark.parametrize("D", WIDTHS)
def test_batched_decode_of_two_streams_is_refused_and_one_stream_is_the_decode_loop(eng, D):
    t, m = _load(eng, D, 1400 + D)
    lib = eng.lib()
    u64 = C.c_uint64
    m.forward(_toks(T, D), eng.MODE_PARRALEL)                   # a history on slots 0 .. 4
    before = _snapshot(m)
    out = (u64 * 64)()
    ft, seeds = (u64 * 2)(11, 12), (u64 * 2)(3, 4)
    assert int(lib.rwkv_decode_batch_greedy(m._h, ft, 2, 4, out)) == E_STATE
    assert "multiple of 64" in lib.rwkv_last_error().decode()
    assert int(lib.rwkv_decode_batch_typical(m._h, ft, 2, 4, 0.9, 0.8, seeds, 0, out)) == E_STATE
    for a, b in zip(before, _snapshot(m)):
        assert np.array_equal(a, b)

    def restore():
        for a, b in zip(m.state.arrays(), before):
            a[:] = b
        m.push_state(MAXT)

    n = 6
    want = m.decode_greedy(11, n)
    after = _snapshot(m)
    restore()
    assert np.array_equal(m.decode_batch_greedy([11], n)[0], want)
    for a, b in zip(after, _snapshot(m)):
        assert np.array_equal(a, b)
    restore()
    want = m.decode_typical(11, n, temp=1.0, tau=0.9, seed=5)
    restore()
    assert np.array_equal(m.decode_batch_typical([11], n, temp=1.0, tau=0.9, seeds=[5])[0], want)
    m.close()


@pytest.mark.parametrize("D", WIDTHS)
def test_stage_chunk_is_refused_and_launches_nothing(eng, D):
    t, m = _load(eng, D, 1500 + D)
    m.forward(_toks(T, D), eng.MODE_GPT)
    before = _snapshot(m)
    logits = m.logits(MAXT).copy()
    with pytest.raises(eng.RWKVError, match=r"multiple of 64.*status -4"):
        m.stage_chunk(_toks(T, 1), T)
    m.sync()
    for a, b in zip(before, _snapshot(m)):
        assert np.array_equal(a, b)
    assert np.array_equal(logits, m.logits(MAXT))
    m.close()


def test_pipe_prefill_is_refused_on_a_width_without_the_chunk_path(eng):
    """rwkv_pipe_prefill has the same check behind rwkv_pipe_init: a one-rank transport, as in test_pipeline_gpu.py"""
    t, m = _load(eng, 1040, 1600)
    m.pipe_init(eng.RWKV.pipe_unique_id(), 0, 1)
    before = _snapshot(m)
    with pytest.raises(eng.RWKVError, match=r"multiple of 64.*status -4"):
        m.pipe_prefill(_toks(40, 2), 40)
    for a, b in zip(before, _snapshot(m)):
        assert np.array_equal(a, b)
    m.close()
