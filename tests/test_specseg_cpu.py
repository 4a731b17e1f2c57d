"""Speculative greedy decoding for many streams, as far as a box without a GPU can check it: rwkv_spec_verify_segments is declared, exported and
bound; engine.lookup_streams, the round loop of RWKV.decode_lookup_streams, is driven by a fake verify over a fixed continuation per stream; and
the margin condition of the GPU suite's oracle case is proved here on the oracle alone."""
import ctypes as C
import os

import numpy as np
import pytest

import spec_cases as sc
import specseg_cases as cs
from support import E_ARG, ROOT, rwkv_mod  # noqa: F401


def test_entry_point_is_declared_exported_and_bound(built, rwkv_mod):
    from rwkv_cpp_accelerated_amd import engine
    lib = engine.lib()
    hdr = open(os.path.join(ROOT, "include", "rwkv_mi355x.h")).read()
    assert "rwkv_spec_verify_segments(" in hdr and "rwkv_spec_verify_segments" in engine.ABI_SYMBOLS
    assert len(lib.rwkv_spec_verify_segments.argtypes) == 8 and C.sizeof(engine.SpecSegment) == 16
    assert lib.rwkv_spec_verify_segments(None, None, None, 1, 0, None, None, None) == E_ARG
    assert callable(engine.RWKV.spec_verify_segments) and callable(engine.RWKV.decode_lookup_streams) and callable(rwkv_mod.specVerifySegments)
    assert "specVerifySegments(" in open(os.path.join(ROOT, "include", "rwkv.h")).read()


@pytest.mark.parametrize("k", [0, 1, 3, 8, 31])
def test_lookup_streams_gives_every_stream_its_continuation(k):
    from rwkv_cpp_accelerated_amd import engine
    N, n_tokens, pass_rows = 5, 40, 32
    rng = np.random.default_rng(11)
    # stream s: a cycle of 4 + s ids (so the lookup drafter has something to find) with a few ids off the cycle (so some of it is wrong)
    cont = [[int(1 + s * 100 + j % (4 + s)) if rng.random() > 0.15 else int(rng.integers(1000, 2000)) for j in range(n_tokens + 1)] for s in range(N)]
    pos, calls = [0] * N, []

    def verify(segs):
        calls.append([s for s, _, _ in segs])
        assert sum(len(ids) for _, ids, _ in segs) <= pass_rows and len(set(calls[-1])) == len(segs)
        out = []
        for s, ids, nd in segs:
            assert pos[s] < n_tokens and ids[0] == cont[s][pos[s]] and nd == len(ids) - 1 <= min(k, n_tokens - pos[s] - 1), "a stream at its budget leaves the rounds"
            a = sc.accept(ids[1:], cont[s][pos[s] + 1:pos[s] + nd + 2])
            out.append((a, cont[s][pos[s] + a + 1], 0))
            pos[s] += a + 1
        return out

    ids, stats = engine.lookup_streams(verify, [[c[0]] for c in cont], n_tokens, k=k, n=2, pass_rows=pass_rows)
    assert ids.tolist() == [c[1:] for c in cont]
    for s, st in enumerate(stats):                                  # a round emits its accepted ids and one more; a stream is in a round until it is done
        assert st["rounds"] + st["accepted"] == n_tokens and st["accepted"] <= st["drafted"] and st["rounds"] == sum(s in c for c in calls)
    assert (k == 0) == (sum(st["drafted"] for st in stats) == 0) and (k < 3 or sum(st["accepted"] for st in stats) > 0)
    assert len(calls[-1]) < N or k == 0                              # the streams end in different rounds


@pytest.mark.parametrize("L,D", cs.WIDTHS)
def test_margin_condition_on_the_oracle_alone(oracle, L, D):
    """the five-segment case of the GPU suite from the oracle's own start state: every row that is picked has a top-two gap of at least MARGIN"""
    from rwkv_cpp_accelerated_amd import modelfile as mf
    om = oracle.from_tensors(L, D, mf.synthetic_tensors(L, D, seed=cs.SEED + D))
    history = [int(v) for v in np.random.default_rng(D).integers(1, cs.V, cs.MAXT)]     # segment_cases.start_state
    g, starts = [], []
    for slot, n, nd, _ in cs.FIVE:
        st = om.new_state()
        om.forward([history[slot]] + (cs.PROMPT if slot == 0 else []), st)
        starts.append([s.copy() for s in st])
        l, gi = om.forward(cs.certain(slot, n - nd), st)[-1], []
        for _ in range(nd + 1):
            assert cs.gap(l) >= cs.MARGIN, (D, slot, len(gi), cs.gap(l))
            gi.append(sc.pick(l))
            l = om.forward([gi[-1]], st)[0]
        g.append(gi)
    segs, want = cs.plant(cs.FIVE, g)
    for (slot, ids, nd), (a, nx, _), st in zip(segs, want, starts):     # the statement finds what was planted
        assert cs.oracle_verify(om.forward, st, ids, nd)[:2] == (a, nx)
    om.close()
