#!/usr/bin/env python3
"""Lookup decoding with draft trees at 7B shapes: what a round costs in the device loop (rwkv_decode_lookup_trees) against the host loop
(RWKV.decode_lookup_tree_streams) and against the bare round (rwkv_spec_verify_trees of the same rows), and what the tree drafter costs alone.

    python tools/lookup_tree_bench.py [--model 7B] [--shapes 1x3,8x3,8x7,16x3] [--branches 1,3] [--reps 5] [--out profiles/lookup_trees]

tools/lookup_loop_bench.py with trees: one context, synthetic weights; per (N streams, k nodes, branches) the histories are planted from the
streams' own greedy continuation, FULL (every draft id right) and NONE (every round finds a draft whose first id is wrong).  Real-text acceptance
is NOT measured; the two bound a round from both sides.  The legs alternate per round of --reps behind a warm round, every leg from the same start
state: ms per ROUND = the call's wall time over the rounds it ran; median and min .. max; `spread` is the largest max - min among the legs of a
line (a difference inside it is not a difference).
  host    RWKV.decode_lookup_tree_streams: drafts and merges in Python, one rwkv_spec_verify_trees per round with its upload, wait and download
  device  RWKV.decode_lookup_tree_device: one call
  bare    rwkv_spec_verify_trees of N chains of 1 + k rows through the C ABI with prebuilt arrays: the round without drafter or bookkeeping
The host loop and the bare call run kernels this tool's change does not touch (profiles/lookup_trees/isa_compare.txt).
The drafter alone: rwkv_debug_lookup_tree (branches 3) beside rwkv_debug_lookup_draft, one stream at 1 k / 16 k / 64 k ids, the match in the
first window or nowhere: wall time of the CALL (conversion, upload, one launch, download, wait)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from rwkv_cpp_accelerated_amd import engine, modelfile as mf


def stats(v):
    return dict(median=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4))


def fmt(s):
    return f"{s['median']:.3f} ms ({s['min']:.3f} .. {s['max']:.3f})"


def wrong(t):
    return t + 1 if t + 1 < mf.VOCAB else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="7B")
    ap.add_argument("--shapes", default="1x3,8x3,8x7,16x3")
    ap.add_argument("--branches", default="1,3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L, D = mf.SHAPES[args.model]
    max_ctx, n_full, n_none = 64, 48, 12
    lib = engine.lib()
    m = engine.RWKV(resident=True)
    m.loadTensors(L, D, mf.synthetic_tensors_torch(L, D, seed=0), maxGPT=max_ctx)
    torch.cuda.empty_cache()
    line = dict(tool="lookup_tree_bench", model=args.model, n_layers=L, n_embed=D, reps=args.reps, maxGPT=max_ctx, device=torch.cuda.get_device_name(0),
                rounds={}, drafter={})
    text = []

    def say(msg):
        text.append(msg)
        print("[lookup_tree_bench] " + msg, file=sys.stderr, flush=True)

    first = [int(v) for v in np.random.default_rng(3).integers(2, 30000, 16)]
    m.forward(first + first, engine.MODE_PARRALEL)                       # a history on slots 0 .. 31; slots 32 .. 63 keep the start state

    def reset(N):
        for s in range(N):
            m.copy_state(s, 32 + s)
        torch.cuda.synchronize()

    for s in range(32):
        m.copy_state(32 + s, s)
    cont = {}
    for shape in args.shapes.split(","):
        N, k = (int(x) for x in shape.split("x"))
        if N * (k + 1) > max_ctx:
            continue
        if N not in cont:
            reset(N)
            cont[N] = m.decode_lookup_device([[f] for f in first[:N]], n_full, k=1, n=2)[0].tolist()
        c = cont[N]
        plans = dict(
            full=(n_full, [[40001 + s, first[s]] + c[s] + [40001 + s, first[s]] for s in range(N)]),
            none=(n_none, [sum([[([first[s]] + c[s])[i], c[s][i], wrong(c[s][i + 1])] + [7] * (k - 1) for i in range(n_none)], [])
                           + [40001 + s, first[s], wrong(c[s][0])] + [7] * (k - 1) + [40001 + s, first[s]] for s in range(N)]))
        arr = (engine.SpecSegment * N)(*[engine.SpecSegment(s, k + 1, k, 0) for s in range(N)])
        toks = (C.c_uint64 * (N * (k + 1)))(*[t for s in range(N) for t in [first[s]] + [7] * k])
        par = (C.c_uint8 * (N * (k + 1)))(*[max(0, r - 1) for _ in range(N) for r in range(k + 1)])
        acc, nx, em = (C.c_uint32 * N)(), (C.c_uint64 * N)(), (C.c_uint64 * (N * engine.SPEC_MAX_DRAFT))()
        for br in [int(x) for x in args.branches.split(",")]:
            for name, (n_tokens, hist) in plans.items():
                got = {leg: [] for leg in ("host", "device", "bare")}
                seen = {}
                for r in range(args.reps + 1):
                    for leg in got:
                        reset(N)
                        t0 = time.perf_counter()
                        if leg == "bare":
                            for _ in range(8):
                                engine._chk(lib.rwkv_spec_verify_trees(m._h, toks, par, arr, N, 0, acc, nx, None, em))
                            rounds = 8
                        else:
                            ids, st = (m.decode_lookup_tree_streams if leg == "host" else m.decode_lookup_tree_device)(hist, n_tokens, k=k, n=2, branches=br)
                            rounds = max(s["rounds"] for s in st)
                            seen[leg] = (ids.tolist(), st)
                        if r:
                            got[leg].append((time.perf_counter() - t0) * 1e3 / rounds)
                assert seen["host"] == seen["device"], "the two loops disagree"
                st = seen["device"][1]
                res = {leg: stats(v) for leg, v in got.items()}
                res.update(spread_ms=round(max(max(v) - min(v) for v in got.values()), 4), rows=N * (k + 1), rounds=max(s["rounds"] for s in st),
                           drafted=sum(s["drafted"] for s in st), accepted=sum(s["accepted"] for s in st), n_tokens=n_tokens)
                line["rounds"][f"{N}x{k}_b{br}_{name}"] = res
                say(f"N={N} k={k} branches={br} {name} ({res['rows']} rows, {res['rounds']} rounds, {res['accepted']} of {res['drafted']} nodes stood): per round "
                    f"host {fmt(res['host'])}, device {fmt(res['device'])}, bare {fmt(res['bare'])}, spread {res['spread_ms']:.3f} ms")
    # ---- the drafters alone ----
    for length in (1024, 16384, 65536):
        for where in ("first_window", "no_match"):
            h = [int(v) for v in np.random.default_rng(length).integers(100, 50000, length)]       # (a bigram repeats by chance once in 4e4 tries)
            if where == "first_window":
                h[length - 40:length - 38] = h[-2:]
            ids, lens = (C.c_uint64 * length)(*h), (C.c_uint64 * 1)(length)
            draft, par8, nd = (C.c_uint64 * 8)(), (C.c_int32 * 8)(), (C.c_uint32 * 1)()
            got = dict(tree=[], chain=[])
            for r in range(args.reps * 4 + 1):
                for leg in got:
                    t0 = time.perf_counter()
                    if leg == "tree":
                        engine._chk(lib.rwkv_debug_lookup_tree(m._h, ids, lens, 1, 8, 2, 3, draft, par8, nd))
                    else:
                        engine._chk(lib.rwkv_debug_lookup_draft(m._h, ids, lens, 1, 8, 2, draft, nd))
                    if r:
                        got[leg].append((time.perf_counter() - t0) * 1e3)
                    assert (nd[0] > 0) == (where == "first_window")
            line["drafter"][f"{length}_{where}"] = {leg: stats(v) for leg, v in got.items()}
            say(f"drafter call, {length} ids, {where}: tree {fmt(stats(got['tree']))}, chain {fmt(stats(got['chain']))}")
    line["resident_bytes"] = m.resident_bytes()
    m.close()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "lookup_tree_bench.json"), "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")
        with open(os.path.join(args.out, "lookup_tree_bench.txt"), "w") as f:
            f.write("\n".join(text) + "\n")
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
