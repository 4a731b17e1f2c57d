#!/usr/bin/env python3
"""The speculative verify and the lookup loops at 7B shapes, this tree against the parent commit, entry point by entry point.

    python tools/spectree_bench.py --parent-lib <librwkv_mi355x.so of the parent commit> [--model 7B] [--shapes 8x3,16x3] [--lookup-shapes 8x3,8x7,16x3]
                                   [--reps 5] [--iters 8] [--parent-first] [--out profiles/spec_one_path] [--name spectree_bench]
    rocprofv3 --kernel-trace --stats ... -- python tools/spectree_bench.py --parent-lib ... --kernels 50      (the per-kernel comparison)

Two contexts in one process with the same synthetic weights, as tools/specseg_bench.py: this tree's library and the parent commit's (--parent-lib),
so that the legs alternate inside one run.  Per shape N x k (N streams, k draft rows each, N (k + 1) rows in one pass), `_parent` the parent's
library and `_this` this tree's:
  chain_parent / chain_this     rwkv_spec_verify_segments
  sample_parent / sample_this   rwkv_spec_sample_segments, every segment a nucleus pick
  chain_tree                    this tree's rwkv_spec_verify_trees with parent[r] = r - 1: the same rows as chain_this through the other entry point
  tree_b2_parent / tree_b2      rwkv_spec_verify_trees of the same rows as real trees: every node has up to 2 children, filled level by level
  tree_b3                       the same with up to 3 children
and per --lookup-shapes, in ms per ROUND (the call's wall time over the rounds its stats report), every call from the same start state (restored
on the device, outside the clock), histories that repeat so that every stream drafts in its first round:
  streams_parent / streams_this rwkv_decode_lookup_streams, n = 2
  trees_parent / trees_this     rwkv_decode_lookup_trees, n = 2, branches = 3
EVERY leg is the C entry point itself on arrays built once, outside the timed loop: no leg pays marshalling another does not.  --parent-first
creates the parent's context before this tree's (the `unchanged` legs with the order swapped: what belongs to the context and not to the build).
--kernels N: no timing; N calls each of rwkv_spec_verify_segments and of the tree call on the same chain rows, of the first shape and of both
libraries, for a kernel trace around the process (the parent's chain call runs k_specseg_wkv as it was, its tree call k_spectree_wkv; this tree's
calls both run the one k_specseg_wkv).
Random drafts: nothing stands (the commit moves the same bytes whatever stands).  The `unchanged` legs time rwkv_decode_greedy (256 ids),
rwkv_forward(GPT, 32) and rwkv_forward(PARRALEL, 32) of both libraries.  --reps rounds of the legs in turn behind a warm round; a round is --iters
calls; ms per call, median and min .. max; `spread` is the largest max - min among the legs of a line (measuring-on-mi355x: a difference inside it
is not a difference); `parent_spread` is that of the parent's own legs alone.  Wall clock around synchronous calls.  Synthetic weights: ACCEPTANCE
ON REAL TEXT IS NOT MEASURED HERE."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

from rwkv_cpp_accelerated_amd import engine, modelfile as mf
import specseg_bench as sb


class Parent:
    """the parent commit's library: the entry points the legs need, bound by hand (this tree's binding asks for symbols it does not have)"""

    def __init__(self, path, L, D, tensors, max_ctx):
        vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
        lib = self.lib = C.CDLL(path)
        lib.rwkv_create.argtypes = [C.POINTER(vp), i32]
        lib.rwkv_load_tensors.argtypes = [vp, u64, u64, C.POINTER(vp), i32, u64]
        lib.rwkv_forward.argtypes = [vp, C.POINTER(u64), u64, i32]
        lib.rwkv_decode_greedy.argtypes = [vp, u64, u64, C.POINTER(u64)]
        for name in ("rwkv_spec_verify_segments", "rwkv_spec_sample_segments", "rwkv_spec_verify_trees", "rwkv_decode_lookup_streams", "rwkv_decode_lookup_trees",
                     "rwkv_state_copy"):      # (the C ABI did not change: this tree's argument lists)
            getattr(lib, name).argtypes = getattr(engine.lib(), name).argtypes
        lib.rwkv_free.argtypes = [vp]; lib.rwkv_free.restype = None
        self.h = vp()
        engine._chk(lib.rwkv_create(C.byref(self.h), 0))
        ptrs = (vp * mf.N_TENSORS)()
        for i, t in enumerate(tensors):
            ptrs[i] = None if t is None else t.data_ptr()
        torch.cuda.synchronize()
        engine._chk(lib.rwkv_load_tensors(self.h, L, D, ptrs, 1, max_ctx))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--model", default="7B")
    ap.add_argument("--shapes", default="8x3,16x3")
    ap.add_argument("--lookup-shapes", default="8x3,8x7,16x3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--name", default="spectree_bench")
    ap.add_argument("--parent-first", action="store_true")
    ap.add_argument("--kernels", type=int, default=0)
    args = ap.parse_args()
    L, D = mf.SHAPES[args.model]
    max_ctx = 64
    lib = engine.lib()
    t = mf.synthetic_tensors_torch(L, D, seed=0)
    parent = Parent(os.path.abspath(args.parent_lib), L, D, t, max_ctx) if args.parent_first else None
    m = engine.RWKV(resident=True)
    m.loadTensors(L, D, t, maxGPT=max_ctx)
    parent = parent or Parent(os.path.abspath(args.parent_lib), L, D, t, max_ctx)
    del t
    torch.cuda.empty_cache()
    line = dict(tool="spectree_bench", model=args.model, n_layers=L, n_embed=D, reps=args.reps, iters=args.iters, maxGPT=max_ctx,
                created_first="parent" if args.parent_first else "this_tree", unchanged={}, verify={}, lookup={})
    text = []

    def say(msg):
        text.append(msg)
        print("[spectree_bench] " + msg, file=sys.stderr, flush=True)

    rng = np.random.default_rng(3)
    ids = lambda n: [int(v) for v in rng.integers(2, mf.VOCAB, n)]
    r32 = ids(32)
    for name, mk, iters, per in (() if args.kernels else (
            ("decode_greedy_256", lambda l, h: sb.greedy_of(l, h, 256), 1, 256), ("forward_gpt32", lambda l, h: sb.forward_of(l, h, r32, engine.MODE_GPT), args.iters, 1),
            ("forward_par32", lambda l, h: sb.forward_of(l, h, r32, engine.MODE_PARRALEL), args.iters, 1))):
        r, spread = sb.alternate(dict(parent=mk(parent.lib, parent.h), this_tree=mk(lib, m._h)), args.reps, iters, per)
        r["spread_ms"] = spread
        line["unchanged"][name] = r
        say(f"unchanged {name}: parent {sb.fmt(r['parent'])}, this tree {sb.fmt(r['this_tree'])}: x{r['this_tree']['median'] / r['parent']['median']:.3f}, spread {spread:.3f} ms")
    both = dict(parent=(parent.lib, parent.h), this=(lib, m._h))
    parent_spread = lambda r: round(max(v["max"] - v["min"] for leg, v in r.items() if leg.endswith("parent")), 4)
    for N, k in [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]:
        rows = [list(dict.fromkeys(ids(3 * (k + 1))))[:k + 1] for _ in range(N)]          # distinct ids per segment: siblings differ whatever the shape
        T = N * (k + 1)
        arr = (engine.SpecSegment * N)(*[engine.SpecSegment(s, k + 1, k, 0) for s in range(N)])
        toks = (C.c_uint64 * T)(*[t for r in rows for t in r])
        acc, nx, row, em = (C.c_uint32 * N)(), (C.c_uint64 * N)(), (C.c_uint64 * N)(), (C.c_uint64 * (N * engine.SPEC_MAX_DRAFT))()
        par = {b: (C.c_uint8 * T)(*([0] + [j // max(b, 1) if b else j for j in range(k)]) * N) for b in (0, 2, 3)}     # 0: the chain; b: row j + 1 below row j // b
        picks = (engine.Pick * N)(*[engine.pick_of("nucleus", temp=1.0, top_p=0.9) for _ in range(N)])
        seeds, step0 = (C.c_uint64 * N)(*range(1, N + 1)), (C.c_uint64 * N)()
        segments_of = lambda l, h: lambda: engine._chk(l.rwkv_spec_verify_segments(h, toks, arr, N, 0, acc, nx, row))
        sample_of = lambda l, h: lambda: engine._chk(l.rwkv_spec_sample_segments(h, toks, arr, N, picks, seeds, step0, 0, acc, nx, row))
        trees_of = lambda l, h, b: lambda: engine._chk(l.rwkv_spec_verify_trees(h, toks, par[b], arr, N, 0, acc, nx, row, em))
        if args.kernels:
            for l, h in both.values():
                for fn in (segments_of(l, h), trees_of(l, h, 0)):
                    for _ in range(args.kernels):
                        fn()
            break
        legs = dict(chain_parent=segments_of(*both["parent"]), chain_this=segments_of(*both["this"]), sample_parent=sample_of(*both["parent"]),
                    sample_this=sample_of(*both["this"]), chain_tree=trees_of(*both["this"], 0), tree_b2_parent=trees_of(*both["parent"], 2),
                    tree_b2=trees_of(*both["this"], 2), tree_b3=trees_of(*both["this"], 3))
        legs["tree_b2"]()
        assert not any(acc), "a random draft stood"
        r, spread = sb.alternate(legs, args.reps, args.iters)
        pspread = parent_spread(r)
        r.update(spread_ms=spread, parent_spread_ms=pspread, rows=T)
        line["verify"][f"{N}x{k}"] = r
        say(f"N={N} k={k} ({T} rows): " + ", ".join(f"{leg} {sb.fmt(r[leg])}" for leg in legs) + f"; spread {spread:.3f} ms, of the parent's legs {pspread:.3f} ms; "
            f"chain_this - chain_parent {r['chain_this']['median'] - r['chain_parent']['median']:+.4f} ms")
    for N, k in [] if args.kernels else [tuple(int(x) for x in s.split("x")) for s in args.lookup_shapes.split(",")]:
        n_tokens, period = 12, 6
        hist = [[int(v) for v in rng.integers(2, 30000, period)] * 4 for _ in range(N)]
        flat, lens = (C.c_uint64 * (N * period * 4))(*[t for h in hist for t in h]), (C.c_uint64 * N)(*[period * 4] * N)
        out, st = (C.c_uint64 * (N * n_tokens))(), (engine.SpecStats * N)()
        lp, tp = engine.LookupParams(k, 2, 0, 0), engine.LookupTreeParams(k, 2, 3, 0)

        def loop_of(l, h, trees):
            def fn():
                for s in range(N):
                    engine._chk(l.rwkv_state_copy(h, s, 32 + s))      # slots 32 .. hold the start state: no leg writes them
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                engine._chk((l.rwkv_decode_lookup_trees if trees else l.rwkv_decode_lookup_streams)(h, flat, lens, N, n_tokens, C.byref(tp if trees else lp), out, st))
                return (time.perf_counter() - t0) * 1e3 / max(x.rounds for x in st), list(out), [(x.rounds, x.drafted, x.accepted) for x in st]
            return fn
        legs = {f"{form}_{who}": loop_of(*both[who], form == "trees") for form in ("streams", "trees") for who in ("parent", "this")}
        got, seen = {leg: [] for leg in legs}, {}
        for rnd in range(args.reps + 1):
            for leg, fn in legs.items():
                ms, ids_out, stats = fn()
                seen[leg] = (ids_out, stats)
                if rnd:
                    got[leg].append(ms)
        for form in ("streams", "trees"):
            assert seen[form + "_parent"] == seen[form + "_this"], f"{form}: the two libraries disagree"
        r = {leg: sb.stats(v) for leg, v in got.items()}
        spread, pspread = round(max(max(v) - min(v) for v in got.values()), 4), parent_spread(r)
        r.update(spread_ms=spread, parent_spread_ms=pspread, rows=N * (k + 1), n_tokens=n_tokens,
                 rounds={form: max(x[0] for x in seen[form + "_this"][1]) for form in ("streams", "trees")},
                 accepted={form: sum(x[2] for x in seen[form + "_this"][1]) for form in ("streams", "trees")})
        line["lookup"][f"{N}x{k}"] = r
        say(f"lookup N={N} k={k} ({r['rows']} rows, rounds {r['rounds']}, accepted {r['accepted']}), ms per round: " + ", ".join(f"{leg} {sb.fmt(r[leg])}" for leg in legs)
            + f"; spread {spread:.3f} ms, of the parent's legs {pspread:.3f} ms; ids and stats equal in both libraries")
    line["resident_bytes"] = m.resident_bytes()
    parent.lib.rwkv_free(parent.h)
    m.close()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, args.name + ".json"), "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")
        with open(os.path.join(args.out, args.name + ".txt"), "w") as f:
            f.write("\n".join(text) + "\n")
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
