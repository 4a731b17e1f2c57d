"""Lookup decoding with draft trees as one device loop (include/rwkv_mi355x.h rwkv_decode_lookup_trees, csrc/lookuptree.hip.h).  The drafter alone
is held to engine.ngram_draft_tree, exactly, on histories planted around the kernel's window of W = 4096 candidate starts and around the trie's
node cap; the loop is held to the host loop RWKV.decode_lookup_tree_streams from the same start state: equal ids, equal stats, the slots' state bit
for bit, and with branches=1 to the chain loop decode_lookup_device.  Everything is integers or bit patterns: no tolerances.  Models:
modelfile.synthetic_tensors at the widths of tests/specseg_cases.py, max_ctx 80."""
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
A, B, X = [5, 6, 7, 8], [5, 6, 9, 1], [5, 4, 0, 2]       # continuations that share a prefix and then diverge
CAP = 6                                           # index of the planted case whose ten continuations differ from their first id on


@pytest.fixture(scope="module")
def bare(eng):
    m = eng.RWKV(resident=True)                   # the drafter needs no model: a created context will do
    yield m
    m.close()


def planted(n):
    """histories of distinct filler ids with the tail (ids 0 and 50276 in it) at the end and at every start of `spots`, {start: the ids behind it}"""
    tail = [(0, V - 1)[(i + n) % 2] for i in range(n)]            # ends with 50276
    out = []
    for length, spots in ((W - 1, {0: A}), (W, {0: A}), (W + 1, {0: A}), (2 * W + n, {0: A}),      # lengths around the window; the only match at start 0
                          (2 * W + n, {W - 1: A}), (2 * W + n, {W - n + 1: B}),                    # straddling the boundary: found only through the halo
                          (2 * W + n, {W + 10 + 40 * i: [20 + i, 0] for i in range(10)}),          # CAP: ten matches in one window, ten first ids
                          (2 * W + n, {100: A, W - 50: B, W + 20: X, W + 300: [0, 3]}),            # two matches in either window: the order across the boundary
                          (2 * W + n, {5: A, W + 7: A}), (300, {10: A, 60: B, 110: X}),            # identical continuations; a shared prefix that diverges
                          (W + 50, {W + 50 - 2 * n - 2: []}), (300, {300 - 2 * n: []}),            # runs into the end of the history: a short branch
                          (2 * W + n, {}), (n, {}), (n + 1, {}), (1, {})):                         # no match; len <= n; the shortest histories
        h = list(range(100, 100 + length))
        for s, cont in spots.items():
            for i, t in enumerate(tail + cont):
                if s + i < length:
                    h[s + i] = t
        if length >= n:
            h[length - n:] = tail
        out.append(h)
    return out


@pytest.mark.parametrize("branches", [1, 3, 8])
@pytest.mark.parametrize("k", [1, 7, 31])
@pytest.mark.parametrize("n", [1, 2, 8])
def test_drafter_is_ngram_draft_tree_on_planted_histories(eng, bare, n, k, branches):
    hist = planted(n)
    assert len(hist) >= 16 and len({len(h) for h in hist}) >= 8            # many streams of different lengths in ONE call
    want = [eng.ngram_draft_tree(h, k, n, branches) for h in hist]
    # the planted set holds what it claims.  CAP: min(branches, 10) continuations that share nothing would make that many times k nodes
    assert len(want[CAP][0]) == k and want[CAP][1].count(-1) == min(k, branches)
    assert k < 3 or branches < 2 or any(p >= 0 and par.count(p) >= 2 for _, par in want for p in par)      # a node of two children: the trie merges
    assert all(bool(ids) == (i < 12) for i, (ids, _) in enumerate(want)) and want[8][1][:4] == [-1, 0, 1, 2][:k]      # identical continuations: one path
    got = bare.debug_lookup_tree(hist, k, n, branches)
    for h, g, w in zip(hist, got, want):
        assert g == w, f"n {n} k {k} branches {branches} len {len(h)}"


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
        """trees matter: the bigram (P, first) in front of the id to feed occurred twice -- the OLDER time followed by s % 4 right ids and a wrong
        one (as tests/test_lookup_loop_gpu.py plants), the MOST RECENT time by an id that is neither right nor that wrong one"""
        out = []
        for s in range(N):
            P, g, r = 40000 + s, self.cont[s], s % 4
            assert P not in g and P != self.first[s]
            other = sc.wrong(sc.wrong(g[0]))
            assert other != g[0]
            out.append([P, self.first[s]] + g[:r] + [sc.wrong(g[r])] + [7] * 8 + [P, self.first[s], other] + [7] * 8 + [P, self.first[s]])
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
    k = min(8, PASS_ROWS // N - 1)        # N (k + 1) rows fit one pass: the host loop's `room` never binds, both loops draft with kd = k
    what = f"D{D} N{N} n_tokens {n_tokens} k {k}"
    runs = {}
    for name, call in (("host", lambda: m.decode_lookup_tree_streams(hist, n_tokens, k=k, n=2, branches=3)),
                       ("tree", lambda: m.decode_lookup_tree_device(hist, n_tokens, k=k, n=2, branches=3)),
                       ("chain", lambda: m.decode_lookup_device(hist, n_tokens, k=k, n=2)),
                       ("one", lambda: m.decode_lookup_tree_device(hist, n_tokens, k=k, n=2, branches=1))):
        restore(m, w.start)
        ids, stats = call()
        runs[name] = (ids.tolist(), stats, snapshot(m, MAXT))
    print(what, {name: [sum(s[f] for s in r[1]) for f in ("rounds", "drafted", "accepted")] for name, r in runs.items()})
    for got, ref in (("tree", "host"), ("one", "chain")):
        assert runs[got][0] == runs[ref][0] == [c[:n_tokens] for c in w.cont[:N]], f"{what}: {got}"
        assert runs[got][1] == runs[ref][1], f"{what}: {got}"
        same_state(runs[got][2], runs[ref][2], f"{what}: named slots of {got} against {ref}", slice(0, N))
        same_state(runs[got][2], w.start, f"{what}: slots not named, {got}", slice(N, None))
    if N > 1 and n_tokens > 1 and k >= 2:            # (else one round count, no room for a draft, or no room for a second branch: the case shows nothing)
        stats = runs["tree"][1]
        # every stream's first branch starts with a wrong id, so whatever stands stood on another one
        assert any(s["accepted"] > 0 for s in stats) and any(s["accepted"] < s["drafted"] for s in stats), what
        assert sum(s["accepted"] for s in runs["chain"][1]) < sum(s["accepted"] for s in stats), what
        assert len({s["rounds"] for s in stats}) >= 2, what


def test_pybind_gives_the_ids_of_the_ctypes_call(eng, rwkv_mod, tmp_path_factory):
    path = model_file(tmp_path_factory, "lookuptree", 3, 64, 4100)
    hist = [[3, 4, 5, 3, 4, 6, 3, 4], [9, 8, 9, 8, 9], [77]]
    h = rwkv_mod.initRwkv()
    rwkv_mod.loadModel(h, path, 16)
    rwkv_mod.setResident(h, True)
    ids, stats = rwkv_mod.decodeLookupTrees(h, hist, 10, 4, 2, 3)
    rwkv_mod.freeRwkv(h)
    m = eng.RWKV(resident=True)
    m.loadFile(path, 16)
    want, want_stats = m.decode_lookup_tree_device(hist, 10, k=4, n=2, branches=3)
    m.close()
    assert ids == want.tolist() and [tuple(s.values()) for s in want_stats] == stats


H5, L5 = [5, 6, 7, 5, 6], [3, 2]                  # two streams: [5, 6, 7], [5, 6]
REFUSED = [      # (context, history, hist_len, n_streams, n_tokens, (k, n, branches, flags), which pointer is NULL, status, text)
    ("M", H5, L5, 2, 4, (4, 2, 0, 0), None, E_ARG, "branches = 0"),
    ("M", H5, L5, 2, 4, (4, 2, 9, 0), None, E_ARG, "branches = 9"),
    ("M", H5, L5, 2, 4, (4, 2, 3, 1), None, E_ARG, "flags must be 0"),
    ("M", H5, L5, 2, 4, (0, 2, 3, 0), None, E_ARG, "k = 0"),
    ("M", H5, L5, 2, 4, (32, 2, 3, 0), None, E_ARG, "k = 32"),
    ("M", H5, L5, 2, 4, (4, 0, 3, 0), None, E_ARG, "n = 0"),
    ("M", H5, L5, 2, 4, (4, 9, 3, 0), None, E_ARG, "n = 9"),
    ("M", H5, L5, 2, 4, (31, 2, 3, 0), None, E_ARG, "ONE pass") if PASS_ROWS == 32 else ("M", H5 * 2 + [1], L5 + [1, 2, 3], 5, 4, (13, 2, 3, 0), None, E_ARG, "ONE pass"),
    ("M", H5, L5, 2, 4, (4, 2, 3, 0), 1, E_ARG, "NULL"),
    ("M", H5, L5, 2, 4, (4, 2, 3, 0), 2, E_ARG, "NULL"),
    ("M", H5, L5, 2, 4, (4, 2, 3, 0), 5, E_ARG, "NULL"),
    ("M", H5, L5, 2, 4, (4, 2, 3, 0), 6, E_ARG, "NULL"),
    ("U", H5, L5, 2, 4, (4, 2, 3, 0), None, E_STATE, "not loaded"),
    ("S", H5, L5, 2, 4, (4, 2, 3, 0), None, E_STATE, "whole-model"),
]


@pytest.fixture(scope="module")
def guard_ctx(eng):
    ctx = GuardContexts(eng, 3, 64, MAXT)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("who,hist,lens,N,n_tokens,params,null,status,text", REFUSED)
def test_refused_calls_leave_state_and_logits_as_they_were(eng, guard_ctx, who, hist, lens, N, n_tokens, params, null, status, text):
    args = [guard_ctx.h[who], (C.c_uint64 * len(hist))(*hist), (C.c_uint64 * len(lens))(*lens), N, n_tokens, C.byref(eng.LookupTreeParams(*params)),
            (C.c_uint64 * 64)(), (eng.SpecStats * 8)()]
    if null is not None:
        args[null] = None
    check_refused(guard_ctx, "rwkv_decode_lookup_trees", args, status, text)
