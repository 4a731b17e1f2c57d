#!/usr/bin/env python3
"""Segmented forward at 7B shapes: what rwkv_forward_segments costs against the parent commit's rwkv_forward on the two layouts it generalises,
and what a continuous-batching server gains from mixing decode rows and prompt pieces behind one read of the weights.

    python tools/segments_bench.py --parent-lib <librwkv_mi355x.so of the parent commit> [--model 7B] [--reps 5] [--iters 8] [--out profiles/segments]

Two contexts in one process with the same synthetic weights: THIS tree's library and the parent commit's (--parent-lib, a second dlopen bound
here to the entry points the legs need), so that the legs alternate inside one run.  Legs, ms per call:
  a   one segment of 32 rows, and one of 64        against the parent's rwkv_forward(GPT) of the same rows
  b   32 segments of length 1, and 64               against the parent's rwkv_forward(PARRALEL)
  c   32 decode rows plus one 32-token prompt piece in ONE call        against the parent's PARRALEL(32) followed by GPT(32)
  d   eight 40-token prompts in ONE call (320 rows, 5 passes)           against eight GPT calls plus eight rwkv_state_copy
a and b show what the plan upload, the segmented instances and the commits cost over the specialised layouts; c and d are the point.
  unchanged_*   rwkv_forward of both builds (GPT 32, GPT 512, PARRALEL 32): the paths this tree does not touch, inside their spread
--reps rounds of (parent, this tree) in turn after a warm round; a round is --iters calls; median and min .. max.  Wall clock around synchronous
calls: every call ends in a stream synchronise."""
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
    """the parent commit's library: rwkv_forward and rwkv_state_copy, bound by hand (this tree's binding asks for symbols it does not have)"""

    def __init__(self, path, L, D, tensors, max_ctx):
        vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
        lib = self.lib = C.CDLL(path)
        assert not hasattr(lib, "rwkv_forward_segments"), "--parent-lib is not the parent's library: it has rwkv_forward_segments"
        lib.rwkv_create.argtypes = [C.POINTER(vp), i32]
        lib.rwkv_load_tensors.argtypes = [vp, u64, u64, C.POINTER(vp), i32, u64]
        lib.rwkv_reset_state.argtypes = [vp]
        lib.rwkv_forward.argtypes = [vp, C.POINTER(u64), u64, i32]
        lib.rwkv_state_copy.argtypes = [vp, u64, u64]
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

    def forward(self, rows, mode):
        self.chk(self.lib.rwkv_forward(self.h, (C.c_uint64 * len(rows))(*rows), len(rows), mode))

    def copy(self, dst, src):
        self.chk(self.lib.rwkv_state_copy(self.h, dst, src))

    def reset(self):
        self.chk(self.lib.rwkv_reset_state(self.h))

    def close(self):
        self.lib.rwkv_free(self.h)


def stats(v):
    return dict(median=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4))


def fmt(s):
    return f"{s['median']:.3f} ms ({s['min']:.3f} .. {s['max']:.3f})"


def timed(fn, per=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3 / per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--model", default="7B")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L, D = mf.SHAPES[args.model]
    max_ctx = 512
    engine.lib()
    t = mf.synthetic_tensors_torch(L, D, seed=0)
    m = engine.RWKV(resident=True)
    m.loadTensors(L, D, t, maxGPT=max_ctx)
    parent = Parent(os.path.abspath(args.parent_lib), L, D, t, max_ctx)
    del t
    torch.cuda.empty_cache()
    line = dict(tool="segments_bench", model=args.model, n_layers=L, n_embed=D, reps=args.reps, iters=args.iters, maxGPT=max_ctx,
                device=torch.cuda.get_device_name(0), legs={})
    text = []

    def say(msg):
        text.append(msg)
        print("[segments_bench] " + msg, file=sys.stderr, flush=True)

    rng = np.random.default_rng(3)
    ids = lambda n: [int(v) for v in rng.integers(2, mf.VOCAB, n)]
    GPT, PAR = engine.MODE_GPT, engine.MODE_PARRALEL

    def leg(name, what, parent_fn, this_fn):
        m.reset_state(); parent.reset()
        legs = dict(parent=parent_fn, segments=this_fn)
        for fn in legs.values():
            fn()
        got = {k: [] for k in legs}
        for _ in range(args.reps):
            for k, fn in legs.items():
                got[k].append(timed(lambda: [fn() for _ in range(args.iters)], args.iters))
        r = {k: stats(v) for k, v in got.items()}
        r["delta_ms"] = round(r["segments"]["median"] - r["parent"]["median"], 4)
        r["ratio"] = round(r["segments"]["median"] / r["parent"]["median"], 4)
        r["spread_ms"] = round(max(max(v) - min(v) for v in got.values()), 4)
        r["what"] = what
        line["legs"][name] = r
        say(f"{name}: {what}: parent {fmt(r['parent'])}, this tree {fmt(r['segments'])}: {r['delta_ms']:+.3f} ms, x{r['ratio']:.3f}, spread {r['spread_ms']:.3f} ms")

    for n in (32, 64):
        rows = ids(n)
        leg(f"a{n}", f"one segment of {n} rows against rwkv_forward(GPT, {n})", lambda: parent.forward(rows, GPT), lambda: m.forward_segments([(0, rows)]))
    for n in (32, 64):
        rows = ids(n)
        segs = [(s, [rows[s]]) for s in range(n)]
        leg(f"b{n}", f"{n} segments of length 1 against rwkv_forward(PARRALEL, {n})", lambda: parent.forward(rows, PAR), lambda: m.forward_segments(segs))
    dec, piece = ids(32), ids(32)
    mixed = [(s, [dec[s]]) for s in range(32)] + [(32, piece)]

    def parent_c():
        parent.forward(dec, PAR); parent.forward(piece, GPT)
    leg("c", "32 decode rows + one 32-token prompt piece in one call against PARRALEL(32) then GPT(32)", parent_c, lambda: m.forward_segments(mixed))
    prompts = [ids(40) for _ in range(8)]
    eight = [(s + 1, p) for s, p in enumerate(prompts)]

    def parent_d():
        for s, p in enumerate(prompts):
            parent.forward(p, GPT); parent.copy(s + 1, 0)
    leg("d", "eight 40-token prompts in one call (320 rows, 5 passes) against eight GPT(40) calls + eight rwkv_state_copy", parent_d, lambda: m.forward_segments(eight))
    # the paths this tree does not change, same process, same alternation: rwkv_forward of both builds
    # (the C entry point of both: RWKV.forward would download the logits rows behind it)
    fwd = engine.lib().rwkv_forward
    for name, n, mode in (("gpt32", 32, GPT), ("gpt512", 512, GPT), ("par32", 32, PAR)):
        rows = ids(n)
        leg("unchanged_" + name, f"rwkv_forward({'GPT' if mode == GPT else 'PARRALEL'}, {n}) of both builds", lambda: parent.forward(rows, mode),
            lambda: engine._chk(fwd(m._h, (C.c_uint64 * n)(*rows), n, mode)))
    line["resident_bytes"] = m.resident_bytes()
    parent.close()
    m.close()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "segments_bench.json"), "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")
        with open(os.path.join(args.out, "segments_bench.txt"), "w") as f:
            f.write("\n".join(text) + "\n")
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
