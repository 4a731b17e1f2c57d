"""Lookup decoding as one device loop (include/rwkv_mi355x.h rwkv_decode_lookup_streams, csrc/lookup.hip.h).  The drafter alone is held to
engine.ngram_draft, exactly, on hand-made histories and on histories planted around the kernel's window of W = 4096 candidate starts; the loop is
held to the host loop RWKV.decode_lookup_streams from the same start state: equal ids, equal stats, and the slots' state bit for bit (the verifier
is the chunk path in both, so no tolerance is involved).  Models: modelfile.synthetic_tensors at the widths of tests/specseg_cases.py, max_ctx 80."""
import ctypes as C
import os

import numpy as np
import pytest

from rwkv_cpp_accelerated_amd import modelfile as mf
import segment_cases as sg
import spec_cases as sc
import specseg_cases as cs
from support import E_ARG, E_STATE, GuardContexts, check_refused, eng, load, model_file, restore, rwkv_mod, same_state, snapshot  # noqa: F401

pytestmark = pytest.mark.gpu
V, MAXT, W = cs.V, cs.MAXT, 4096                  # W: csrc/lookup.hip.h LK_W
PASS_ROWS = 32 if int(os.environ.get("RWKV_SEQ_ROWS", "64")) <= 32 else 64
HAND_MADE = [        # (history, k, n): tests/test_spec_cpu.py::test_ngram_draft_on_hand_made_histories, the calls the device accepts
    ([1, 2, 3, 4, 5], 4, 3), ([1, 2, 3], 4, 3), ([1, 2, 3, 9, 8, 1, 2, 3], 4, 3), ([1, 2, 3, 9, 8, 1, 2, 3], 2, 3), ([7, 1, 2, 3, 1, 2, 3], 4, 3),
    ([5, 5, 5, 5], 4, 3), ([5, 5, 5, 5, 5], 4, 2), ([1, 2, 7, 1, 2, 8, 1, 2], 1, 2), ([1, 2, 7, 1, 2], 3, 2),
]


@pytest.fixture(scope="module")
def bare(eng):
    m = eng.RWKV(resident=True)                   # the drafter needs no model: a created context will do
    yield m
    m.close()


def planted(n):
    """[(history, whether its tail has an earlier occurrence)]: distinct filler ids, the tail (ids 0 and 50276 in it) planted at `starts`, ids 0
    and 50276 behind the first occurrence"""
    tail = [(0, V - 1)[(i + n) % 2] for i in range(n)]            # ends with 50276
    out = []
    for length, starts in ((W - 1, [0]), (W, [0]), (W + 1, [0]), (2 * W + n, [0]),                # lengths around the window; the only match at start 0
                           (2 * W + n, [W - 1]), (2 * W + n, [W - n + 1]),                         # straddling the boundary: found only through the halo
                           (2 * W + n, [5, W + 7]), (2 * W + n, [W + 7, 2 * W - 20]),              # two matches, two windows / one window: the later wins
                           (W + 50, [W + 50 - 2 * n - 2]), (300, [300 - 2 * n]),                   # runs into the tail: a short draft
                           (2 * W + n, []), (n, []), (n + 1, []), (1, [])):                        # no match; len <= n; the shortest histories
        h = list(range(100, 100 + length))
        for s in starts:
            h[s:s + n] = tail
            if s + n + 2 <= length - n:
                h[s + n:s + n + 2] = [0, V - 1] if n > 1 else [0, 9]
        if length >= n:
            h[length - n:] = tail
        out.append((h[:length], bool(starts)))
    return out


@pytest.mark.parametrize("k", [1, 7, 31])
@pytest.mark.parametrize("n", [1, 2, 8])
def test_drafter_is_ngram_draft_on_planted_histories(eng, bare, n, k):
    cases = planted(n) + [(h, None) for h, _, _ in HAND_MADE[:4]]
    hist = [h for h, _ in cases]
    assert len(hist) >= 16 and len({len(h) for h in hist}) >= 10          # many streams of different lengths in ONE call
    want = [eng.ngram_draft(h, k, n) for h in hist]
    for (h, match), w in zip(cases, want):
        assert match is None or bool(w) == match, (len(h), n, k)           # the case plants what it claims
    got = bare.debug_lookup_draft(hist, k, n)
    for h, g, w in zip(hist, got, want):
        assert g == w, f"n {n} k {k} len {len(h)}"


@pytest.mark.parametrize("i", range(len(HAND_MADE)))
def test_drafter_is_ngram_draft_on_hand_made_histories(eng, bare, i):
    h, k, n = HAND_MADE[i]
    assert bare.debug_lookup_draft([h], k, n) == [eng.ngram_draft(h, k, n)]


class Width:
    """one model, its start state, 16 first ids and the greedy continuation of every stream from it (once per module)"""

    def __init__(self, eng, L, D):
        self.m = load(eng, L, D, 0, MAXT, mf.synthetic_tensors(L, D, seed=cs.SEED + D))
        sg.start_state(eng, self.m, D)
        self.start = snapshot(self.m, MAXT)
        self.first = [int(t) for t in np.random.default_rng(D).integers(1, 30000, 16)]
        cont, _ = self.m.decode_lookup_streams([[f] for f in self.first], 12, k=1, n=2)          # nothing to look up: 12 plain rounds
        self.cont = cont.tolist()

    def histories(self, N):
        """as tests/test_spec_gpu.py plants for decode_lookup: in front of the id to feed the bigram (P, first) followed by s % 4 right ids and a
        wrong one -- some drafts stand, some fall, and the streams retire in different rounds"""
        out = []
        for s in range(N):
            P, g, r = 40000 + s, self.cont[s], s % 4
            assert P not in g and P != self.first[s]
            out.append([P, self.first[s]] + g[:r] + [sc.wrong(g[r])] + [7] * 8 + [P, self.first[s]])
        return out


@pytest.fixture(scope="module")
def widths(eng):
    cache = {}

    def get(L, D):
        if (L, D) not in cache:
            cache[(L, D)] = Width(eng, L, D)
        return cache[(L, D)]
    yield get
    for w in cache.values():
        w.m.close()


@pytest.mark.parametrize("n_tokens", [1, 2, 12])
@pytest.mark.parametrize("N", [1, 5, 16])
@pytest.mark.parametrize("L,D", cs.WIDTHS)
def test_loop_is_the_host_loop(eng, widths, L, D, N, n_tokens):
    w = widths(L, D)
    m, hist = w.m, w.histories(N)
    k = min(8, PASS_ROWS // N - 1)        # N (k + 1) rows fit one pass: the host loop's per-round `room` never binds, both loops draft the same kd,
    restore(m, w.start)                   # and only then are the stats comparable
    want, want_stats = m.decode_lookup_streams(hist, n_tokens, k=k, n=2)
    host = snapshot(m, MAXT)
    restore(m, w.start)
    got, stats = m.decode_lookup_device(hist, n_tokens, k=k, n=2)
    what = f"D{D} N{N} n_tokens {n_tokens} k {k}"
    print(what, stats)
    assert got.tolist() == want.tolist() == [c[:n_tokens] for c in w.cont[:N]], what
    assert stats == want_stats, what
    dev = snapshot(m, MAXT)
    same_state(dev, host, what + ": named slots against the host loop", slice(0, N))
    same_state(dev, w.start, what + ": slots not named", slice(N, None))
    if N > 1 and n_tokens > 1:            # (one stream has one round count; one id leaves no room for a draft) -- else the case shows nothing
        assert any(s["accepted"] > 0 for s in stats) and any(s["accepted"] < s["drafted"] for s in stats), what
        assert len({s["rounds"] for s in stats}) >= 2, what


def test_pybind_gives_the_ids_of_the_ctypes_call(eng, rwkv_mod, tmp_path_factory):
    path = model_file(tmp_path_factory, "lookup", 3, 64, 4100)
    hist = [[3, 4, 5, 3, 4, 6, 3, 4], [9, 8, 9, 8, 9], [77]]
    h = rwkv_mod.initRwkv()
    rwkv_mod.loadModel(h, path, 16)
    rwkv_mod.setResident(h, True)
    ids, stats = rwkv_mod.decodeLookupStreams(h, hist, 10, 4, 2)
    rwkv_mod.freeRwkv(h)
    m = eng.RWKV(resident=True)
    m.loadFile(path, 16)
    want, want_stats = m.decode_lookup_device(hist, 10, k=4, n=2)
    m.close()
    assert ids == want.tolist() and [tuple(s.values()) for s in want_stats] == stats


H5, L5 = [5, 6, 7, 5, 6], [3, 2]                  # two streams: [5, 6, 7], [5, 6]
REFUSED = [      # (context, history, hist_len, n_streams, n_tokens, (k, n, flags, reserved), which pointer is NULL, status, text)
    ("M", H5, L5, 2, 4, (0, 2, 0, 0), None, E_ARG, "k = 0"),
    ("M", H5, L5, 2, 4, (32, 2, 0, 0), None, E_ARG, "k = 32"),
    ("M", H5, L5, 2, 4, (4, 0, 0, 0), None, E_ARG, "n = 0"),
    ("M", H5, L5, 2, 4, (4, 9, 0, 0), None, E_ARG, "n = 9"),
    ("M", H5, L5, 2, 4, (31, 2, 0, 0), None, E_ARG, "ONE pass") if PASS_ROWS == 32 else ("M", H5 * 2 + [1], L5 + [1, 2, 3], 5, 4, (13, 2, 0, 0), None, E_ARG, "ONE pass"),
    ("M", H5, [3, 0], 2, 4, (4, 2, 0, 0), None, E_ARG, "hist_len[1] = 0"),
    ("M", [5, 6, V, 5, 6], L5, 2, 4, (4, 2, 0, 0), None, E_ARG, f"token id {V} out of range"),
    ("M", H5, L5, 2, 0, (4, 2, 0, 0), None, E_ARG, "n_tokens must be in 1.."),
    ("M", H5, L5, 0, 4, (4, 2, 0, 0), None, E_ARG, "n_streams must be in 1.."),
    ("M", H5, L5, 2, 4, (4, 2, 1, 0), None, E_ARG, "flags and reserved must be 0"),
    ("M", H5, L5, 2, 4, (4, 2, 0, 1), None, E_ARG, "flags and reserved must be 0"),
    ("M", H5, L5, 2, 4, (4, 2, 0, 0), 1, E_ARG, "NULL"),
    ("M", H5, L5, 2, 4, (4, 2, 0, 0), 2, E_ARG, "NULL"),
    ("M", H5, L5, 2, 4, (4, 2, 0, 0), 5, E_ARG, "NULL"),
    ("M", H5, L5, 2, 4, (4, 2, 0, 0), 6, E_ARG, "NULL"),
    ("U", H5, L5, 2, 4, (4, 2, 0, 0), None, E_STATE, "not loaded"),
    ("S", H5, L5, 2, 4, (4, 2, 0, 0), None, E_STATE, "whole-model"),
]


@pytest.fixture(scope="module")
def guard_ctx(eng):
    ctx = GuardContexts(eng, 3, 64, MAXT)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("who,hist,lens,N,n_tokens,params,null,status,text", REFUSED)
def test_refused_calls_leave_state_and_logits_as_they_were(eng, guard_ctx, who, hist, lens, N, n_tokens, params, null, status, text):
    args = [guard_ctx.h[who], (C.c_uint64 * len(hist))(*hist), (C.c_uint64 * len(lens))(*lens), N, n_tokens, C.byref(eng.LookupParams(*params)),
            (C.c_uint64 * 64)(), (eng.SpecStats * 8)()]
    if null is not None:
        args[null] = None
    check_refused(guard_ctx, "rwkv_decode_lookup_streams", args, status, text)
