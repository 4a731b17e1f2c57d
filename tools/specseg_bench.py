#!/usr/bin/env python3
"""Speculative greedy decoding for many streams at 7B shapes: what rwkv_spec_verify_segments costs per call against the two things the parent
commit already has, and what the parent's own paths cost in this tree.

    python tools/specseg_bench.py --parent-lib <librwkv_mi355x.so of the parent commit> [--model 7B] [--streams 2,4,8,16] [--ks 1,3,7]
                                  [--reps 5] [--iters 8] [--out profiles/spec_streams]

Two contexts in one process with the same synthetic weights: this tree's library and the parent commit's (--parent-lib, a second dlopen bound here
to the entry points the legs need), so that the legs alternate inside one run.  Per (N streams, k drafts) with N (k + 1) rows in one pass:
  step      parent rwkv_forward(PARRALEL) of N rows: the batched decode step that a round of speculation replaces
  segments  rwkv_forward_segments of the same N (k + 1) rows: the pass without checkpoints, picks, accept and commit
  verify    rwkv_spec_verify_segments, every draft wrong at once (the commit moves the same bytes whatever stands)
verify / step is the BREAK-EVEN: the ids a stream must emit per round for the round to cost what plain steps cost.  A round emits k + 1 ids per
stream at full acceptance and 1 with every draft rejected; the drafter's own time is not counted.  verify - segments is what checkpointing and the
commit add.  The `unchanged` legs time rwkv_decode_greedy (256 ids), rwkv_forward(GPT, 32) and rwkv_forward(PARRALEL, 32) of both libraries.
--reps rounds of the legs in turn behind a warm round; a round is --iters calls; ms per call, median and min .. max; `spread` is the largest
max - min among the legs of a line (measuring-on-mi355x: a difference inside it is not a difference).  Wall clock around synchronous calls.
Synthetic weights: ACCEPTANCE ON REAL TEXT IS NOT MEASURED HERE, only what a round costs."""
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


class Parent:
    """the parent commit's library: rwkv_forward and rwkv_decode_greedy, bound by hand (this tree's binding asks for a symbol it does not have)"""

    def __init__(self, path, L, D, tensors, max_ctx):
        vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
        lib = self.lib = C.CDLL(path)
        assert not hasattr(lib, "rwkv_spec_verify_segments"), "--parent-lib is not the parent's library: it has rwkv_spec_verify_segments"
        lib.rwkv_create.argtypes = [C.POINTER(vp), i32]
        lib.rwkv_load_tensors.argtypes = [vp, u64, u64, C.POINTER(vp), i32, u64]
        lib.rwkv_forward.argtypes = [vp, C.POINTER(u64), u64, i32]
        lib.rwkv_decode_greedy.argtypes = [vp, u64, u64, C.POINTER(u64)]
        lib.rwkv_free.argtypes = [vp]; lib.rwkv_free.restype = None
        lib.rwkv_last_error.restype = C.c_char_p
        self.h = vp()
        self.chk(lib.rwkv_create(C.byref(self.h), 0))
        ptrs = (vp * mf.N_TENSORS)()
        for i, t in enumerate(tensors):
            ptrs[i] = None if t is None else t.data_ptr()
        torch.cuda.synchronize()
        self.chk(lib.rwkv_load_tensors(self.h, L, D, ptrs, 1, max_ctx))

    def chk(self, rc):
        if rc != 0:
            raise RuntimeError(self.lib.rwkv_last_error().decode(errors="replace"))


def forward_of(lib, h, rows, mode):
    arr = (C.c_uint64 * len(rows))(*rows)
    return lambda: engine._chk(lib.rwkv_forward(h, arr, len(rows), mode))


def greedy_of(lib, h, n):
    out = (C.c_uint64 * n)()
    return lambda: engine._chk(lib.rwkv_decode_greedy(h, 5, n, out))


def stats(v):
    return dict(median=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4))


def fmt(s):
    return f"{s['median']:.3f} ms ({s['min']:.3f} .. {s['max']:.3f})"


def alternate(legs, reps, iters, per=1):
    """{leg: stats of ms per call (over `per`)}, the legs in turn per round behind a warm round, and the largest max - min"""
    got = {k: [] for k in legs}
    for r in range(reps + 1):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            if r:
                got[k].append((time.perf_counter() - t0) * 1e3 / (iters * per))
    return {k: stats(v) for k, v in got.items()}, round(max(max(v) - min(v) for v in got.values()), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--model", default="7B")
    ap.add_argument("--streams", default="2,4,8,16")
    ap.add_argument("--ks", default="1,3,7")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L, D = mf.SHAPES[args.model]
    max_ctx = 64
    lib = engine.lib()
    t = mf.synthetic_tensors_torch(L, D, seed=0)
    m = engine.RWKV(resident=True)
    m.loadTensors(L, D, t, maxGPT=max_ctx)
    parent = Parent(os.path.abspath(args.parent_lib), L, D, t, max_ctx)
    del t
    torch.cuda.empty_cache()
    line = dict(tool="specseg_bench", model=args.model, n_layers=L, n_embed=D, reps=args.reps, iters=args.iters, maxGPT=max_ctx,
                device=torch.cuda.get_device_name(0), unchanged={}, verify={})
    text = []

    def say(msg):
        text.append(msg)
        print("[specseg_bench] " + msg, file=sys.stderr, flush=True)

    rng = np.random.default_rng(3)
    ids = lambda n: [int(v) for v in rng.integers(2, mf.VOCAB, n)]
    # ---- what the parent already had, both builds ----
    r32 = ids(32)
    for name, mk, iters, per in (("decode_greedy_256", lambda l, h: greedy_of(l, h, 256), 1, 256), ("forward_gpt32", lambda l, h: forward_of(l, h, r32, engine.MODE_GPT), args.iters, 1),
                                 ("forward_par32", lambda l, h: forward_of(l, h, r32, engine.MODE_PARRALEL), args.iters, 1)):
        r, spread = alternate(dict(parent=mk(parent.lib, parent.h), this_tree=mk(lib, m._h)), args.reps, iters, per)
        r["spread_ms"] = spread
        line["unchanged"][name] = r
        d = r["this_tree"]["median"] - r["parent"]["median"]
        say(f"unchanged {name}: parent {fmt(r['parent'])}, this tree {fmt(r['this_tree'])}: {d:+.4f} ms, x{r['this_tree']['median'] / r['parent']['median']:.3f}, spread {spread:.3f} ms")
    # ---- the verify ----
    for N in [int(x) for x in args.streams.split(",")]:
        for k in [int(x) for x in args.ks.split(",")]:
            if N * (k + 1) > max_ctx:
                continue
            segs = [(s, ids(k + 1), k) for s in range(N)]
            legs = dict(step=forward_of(parent.lib, parent.h, [g[1][0] for g in segs], engine.MODE_PARRALEL),
                        segments=lambda: m.forward_segments([(s, i) for s, i, _ in segs]), verify=lambda: m.spec_verify_segments(segs))
            assert all(a == 0 for a, _, _ in m.spec_verify_segments(segs)), "a random draft stood"
            r, spread = alternate(legs, args.reps, args.iters)
            r.update(spread_ms=spread, rows=N * (k + 1), added_ms=round(r["verify"]["median"] - r["segments"]["median"], 4),
                     break_even_ids=round(r["verify"]["median"] / r["step"]["median"], 3))
            r["speedup_full_acceptance"] = round((k + 1) / r["break_even_ids"], 3)
            r["speedup_all_rejected"] = round(1 / r["break_even_ids"], 3)
            line["verify"][f"{N}x{k}"] = r
            say(f"N={N} k={k} ({r['rows']} rows): step of {N} rows {fmt(r['step'])}, segments {fmt(r['segments'])}, verify {fmt(r['verify'])} "
                f"(added {r['added_ms']:+.3f} ms), spread {spread:.3f} ms; break-even {r['break_even_ids']:.2f} ids per stream and round; "
                f"x{r['speedup_full_acceptance']:.2f} at full acceptance, x{r['speedup_all_rejected']:.2f} with every draft rejected")
    line["resident_bytes"] = m.resident_bytes()
    parent.lib.rwkv_free(parent.h)
    m.close()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "specseg_bench.json"), "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")
        with open(os.path.join(args.out, "specseg_bench.txt"), "w") as f:
            f.write("\n".join(text) + "\n")
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
