#!/usr/bin/env python3
"""What rwkv_sample_rows and rwkv_spec_sample_segments cost, against what the parent commit has for the same work.

    python tools/pick_rows_bench.py --parent-lib <librwkv_mi355x.so of the parent commit> [--qs 8,32,64] [--model 7B] [--reps 7] [--iters 8]
                                    [--out profiles/pick_rows]

Two contexts per part in one process, this tree's library and the parent's (--parent-lib, a second dlopen bound by hand), so that the legs
alternate inside one run.
SAMPLER (the sampler depends on V only: a 2-layer model of width 256), per Q and parameter set (top-p alone; top-k 40 with penalties, counted):
  rows      ONE rwkv_sample_rows call of Q nucleus queries on Q distinct rows and slots
  calls     the parent's Q synchronous calls of rwkv_sample_nucleus on the same rows and slots
  loop      the per-step cost of the sampler in the parent's rwkv_decode_batch_nucleus(Q streams): (a 32-step nucleus call - a 32-step
            rwkv_decode_batch_greedy call) / 32.  The greedy pick it replaces is not added back, so this is a lower bound of the
            consecutive-row sampler's step cost; device time only, no upload or download per step: the specialised layout the new call generalises
  rows - loop is what generality costs per call (the record upload, the id download, one synchronisation, the table reads).
VERIFY (--model shapes): rwkv_spec_sample_segments (nucleus picks) against the parent's rwkv_spec_verify_segments on the same rows, every draft
wrong at once: 8 x 3 drafts (32 rows) and 16 x 3 (64 rows).
--reps rounds of the legs in turn behind a warm round, --iters calls per round; ms per call: median (min .. max); `spread` is the largest
max - min among the legs of a line: a difference inside it is not a difference.  Wall clock around synchronous calls."""
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
    """the parent commit's library, bound by hand to the entry points the legs need"""

    def __init__(self, path, L, D, tensors, max_ctx):
        vp, u64, i32, u32 = C.c_void_p, C.c_uint64, C.c_int, C.c_uint32
        lib = self.lib = C.CDLL(path)
        assert not hasattr(lib, "rwkv_sample_rows"), "--parent-lib is not the parent's library: it has rwkv_sample_rows"
        lib.rwkv_create.argtypes = [C.POINTER(vp), i32]
        lib.rwkv_load_tensors.argtypes = [vp, u64, u64, C.POINTER(vp), i32, u64]
        lib.rwkv_forward.argtypes = [vp, C.POINTER(u64), u64, i32]
        lib.rwkv_sample_nucleus.argtypes = [vp, u64, u64, C.POINTER(engine.NucleusParams), C.c_double, C.POINTER(u64)]
        lib.rwkv_decode_batch_nucleus.argtypes = [vp, C.POINTER(u64), u64, u64, C.POINTER(engine.NucleusParams), C.POINTER(u64), C.POINTER(u64)]
        lib.rwkv_decode_batch_greedy.argtypes = [vp, C.POINTER(u64), u64, u64, C.POINTER(u64)]
        lib.rwkv_spec_verify_segments.argtypes = [vp, C.POINTER(u64), C.POINTER(engine.SpecSegment), u64, u32, C.POINTER(u32), C.POINTER(u64), C.POINTER(u64)]
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


def stats(v):
    return dict(median=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4))


def fmt(s):
    return f"{s['median']:.3f} ms ({s['min']:.3f} .. {s['max']:.3f})"


def alternate(legs, reps, iters):
    """{leg: stats of ms per call}, the legs in turn per round behind a warm round, and the largest max - min"""
    got = {k: [] for k in legs}
    for r in range(reps + 1):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            if r:
                got[k].append((time.perf_counter() - t0) * 1e3 / iters)
    return {k: stats(v) for k, v in got.items()}, round(max(max(v) - min(v) for v in got.values()), 4)


def pair(L, D, max_ctx):
    t = mf.synthetic_tensors_torch(L, D, seed=0)
    m = engine.RWKV(resident=True)
    m.loadTensors(L, D, t, maxGPT=max_ctx)
    return m, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--qs", default="8,32,64")
    ap.add_argument("--model", default="7B")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    line = dict(tool="pick_rows_bench", reps=args.reps, iters=args.iters, device=torch.cuda.get_device_name(0), sampler={}, verify={})
    text = []

    def say(msg):
        text.append(msg)
        print("[pick_rows_bench] " + msg, file=sys.stderr, flush=True)

    rng = np.random.default_rng(3)
    ids = lambda n: [int(v) for v in rng.integers(2, mf.VOCAB, n)]
    u64 = C.c_uint64
    # ---- the sampler ----
    STEPS, max_ctx = 32, 64
    m, t = pair(2, 256, max_ctx)
    parent = Parent(os.path.abspath(args.parent_lib), 2, 256, t, max_ctx)
    for Q in [int(x) for x in args.qs.split(",")]:
        first = ids(Q)
        arr = (u64 * Q)(*first)
        for ctx_lib, h in ((engine.lib(), m._h), (parent.lib, parent.h)):          # Q logits rows, and counts on Q slots
            engine._chk(ctx_lib.rwkv_forward(h, arr, Q, engine.MODE_PARRALEL))
        for name, kw in (("top_p", dict(temp=1.0, top_p=0.9)), ("top_k_penalties", dict(temp=0.8, top_p=0.9, top_k=40, presence=0.4, frequency=0.4, decay=0.996))):
            p = engine.nucleus_params(**kw)
            qs = [engine.pick_query(r, r, u=0.1 + 0.8 * r / Q, **kw) for r in range(Q)]
            tok, out, seeds = u64(0), (u64 * (Q * STEPS))(), (u64 * Q)(*range(Q))

            def calls():
                for q in qs:
                    parent.chk(parent.lib.rwkv_sample_nucleus(parent.h, q.row, q.slot, C.byref(p), q.u, C.byref(tok)))
            legs = dict(rows=lambda: m.sample_rows(qs), calls=calls,
                        loop_nucleus=lambda: parent.chk(parent.lib.rwkv_decode_batch_nucleus(parent.h, arr, Q, STEPS, C.byref(p), seeds, out)),
                        loop_greedy=lambda: parent.chk(parent.lib.rwkv_decode_batch_greedy(parent.h, arr, Q, STEPS, out)))
            r, spread = alternate(legs, args.reps, args.iters)
            loop = (r["loop_nucleus"]["median"] - r["loop_greedy"]["median"]) / STEPS
            r.update(spread_ms=spread, loop_step_ms=round(loop, 4), generality_ms=round(r["rows"]["median"] - loop, 4),
                     speedup_over_calls=round(r["calls"]["median"] / r["rows"]["median"], 2))
            line["sampler"][f"Q{Q}_{name}"] = r
            say(f"Q={Q} {name}: one sample_rows call {fmt(r['rows'])}; parent's {Q} sample_nucleus calls {fmt(r['calls'])} (x{r['speedup_over_calls']:.2f}); "
                f"sampler step inside the parent's decode_batch_nucleus {loop:.3f} ms ({STEPS}-step nucleus {fmt(r['loop_nucleus'])} - greedy {fmt(r['loop_greedy'])}); "
                f"generality {r['generality_ms']:+.3f} ms per call; spread {spread:.3f} ms")
            for ctx_lib, h in ((engine.lib(), m._h), (parent.lib, parent.h)):      # the loops moved the rows: plant them again
                engine._chk(ctx_lib.rwkv_forward(h, arr, Q, engine.MODE_PARRALEL))
    parent.lib.rwkv_free(parent.h)
    m.close()
    del t
    torch.cuda.empty_cache()
    # ---- the verify ----
    L, D = mf.SHAPES[args.model]
    m, t = pair(L, D, 64)
    parent = Parent(os.path.abspath(args.parent_lib), L, D, t, 64)
    del t
    torch.cuda.empty_cache()
    for N, k in ((8, 3), (16, 3)):
        segs = [(s, ids(k + 1), k) for s in range(N)]
        sarr = (engine.SpecSegment * N)(*[engine.SpecSegment(s, k + 1, k, 0) for s in range(N)])
        toks = (u64 * (N * (k + 1)))(*[i for _, g, _ in segs for i in g])
        acc, nx, row = (C.c_uint32 * N)(), (u64 * N)(), (u64 * N)()
        picks, seeds, step0 = [engine.pick_of(temp=0.8, top_p=0.9, top_k=40)] * N, list(range(N)), [0] * N
        legs = dict(greedy_parent=lambda: parent.chk(parent.lib.rwkv_spec_verify_segments(parent.h, toks, sarr, N, 0, acc, nx, row)),
                    greedy=lambda: m.spec_verify_segments(segs), sampled=lambda: m.spec_sample_segments(segs, picks, seeds, step0))
        r, spread = alternate(legs, args.reps, args.iters)
        r.update(spread_ms=spread, rows=N * (k + 1), queries=N * (k + 1), added_ms=round(r["sampled"]["median"] - r["greedy_parent"]["median"], 4))
        line["verify"][f"{N}x{k}"] = r
        say(f"{args.model} N={N} k={k} ({r['rows']} rows): parent's spec_verify_segments {fmt(r['greedy_parent'])}, this tree's {fmt(r['greedy'])}, "
            f"spec_sample_segments {fmt(r['sampled'])}: {r['added_ms']:+.3f} ms for sampling {r['queries']} rows; spread {spread:.3f} ms")
    line["resident_bytes"] = m.resident_bytes()
    parent.lib.rwkv_free(parent.h)
    m.close()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "pick_rows_bench.json"), "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")
        with open(os.path.join(args.out, "pick_rows_bench.txt"), "w") as f:
            f.write("\n".join(text) + "\n")
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
