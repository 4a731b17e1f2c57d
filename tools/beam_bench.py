#!/usr/bin/env python3
"""Beam search at 7B shapes: what the selection across rows and the state gather cost per step, against what a caller had before them.

    python tools/beam_bench.py --parent-lib <librwkv_mi355x.so of the parent commit> [--model 7B] [--widths 4,8,16] [--steps 32] [--reps 5]
                               [--rotations 20] [--out profiles/beam]

Two contexts in one process, the same synthetic weights in both: THIS tree's library (through the Python engine) and the parent commit's
(--parent-lib, a second dlopen bound here to the handful of entry points the legs need), so that the legs alternate inside one run.  Per width W:
  (A) parent_logprobs  rwkv_decode_batch_logprobs(greedy, N = W, top_n = W + 1) of the PARENT library: the nearest loop that existed -- the same
                       PARRALEL step and the same two top-n launches, a greedy pick in place of the selection, no gather
  (B) beam             rwkv_decode_beam(W): (B) - (A) is what the selection and the gather cost per step
  (C) parent_copies    a full rotation of W slots the way a caller restated it on the parent: W + 1 rwkv_state_copy calls through a spare slot
  (D) permute          rwkv_state_permute of the same rotation: every slot moves, 40 W L D bytes read and written twice (staging and back)
--reps rounds of A, B, C, D in turn after one warm round of each; a round of (A) / (B) is one call of --steps steps, of (C) / (D) --rotations
rotations.  Median and min .. max of ms per step (ms per rotation), the spread of each pair, and one JSON line on stdout; with --out the same as
beam_bench.json / beam_bench.txt in that directory.  Wall clock around synchronous calls: every leg ends in a stream synchronise."""
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
    """the parent commit's library: the entry points of legs (A) and (C), bound by hand (this tree's binding asks for symbols it does not have)"""

    def __init__(self, path, L, D, tensors, max_ctx):
        vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
        lib = self.lib = C.CDLL(path)
        assert not hasattr(lib, "rwkv_decode_beam"), "--parent-lib is not the parent's library: it has rwkv_decode_beam"
        lib.rwkv_create.argtypes = [C.POINTER(vp), i32]
        lib.rwkv_load_tensors.argtypes = [vp, u64, u64, C.POINTER(vp), i32, u64]
        lib.rwkv_reset_state.argtypes = [vp]
        lib.rwkv_state_copy.argtypes = [vp, u64, u64]
        lib.rwkv_free.argtypes = [vp]; lib.rwkv_free.restype = None
        lib.rwkv_last_error.restype = C.c_char_p
        lib.rwkv_decode_batch_logprobs.argtypes = [vp, C.POINTER(u64), u64, u64, C.POINTER(engine.Pick), C.POINTER(u64), C.POINTER(engine.StopParams),
                                                   C.POINTER(engine.LogprobOut), C.POINTER(u64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(u64)]
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

    def logprobs(self, first, steps, top_n):
        n = len(first)
        e = n * steps
        lp, tid, tlp = np.zeros(e), np.zeros(e * top_n, np.uint64), np.zeros(e * top_n)
        dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
        rec = engine.LogprobOut(top_n, 0, lp.ctypes.data_as(dp), None, tid.ctypes.data_as(up), tlp.ctypes.data_as(dp))
        pk = engine.Pick(engine.PICK_GREEDY, 1.0, 0.8, 0, engine.nucleus_params())
        out = (C.c_uint64 * e)()
        self.chk(self.lib.rwkv_decode_batch_logprobs(self.h, (C.c_uint64 * n)(*first), n, steps, C.byref(pk), None, None, C.byref(rec), out, None, None, None))

    def rotate(self, W):
        """slot m <- slot m + 1 (mod W) through the spare slot W"""
        self.chk(self.lib.rwkv_state_copy(self.h, W, 0))
        for m in range(W - 1):
            self.chk(self.lib.rwkv_state_copy(self.h, m, m + 1))
        self.chk(self.lib.rwkv_state_copy(self.h, W - 1, W))

    def close(self):
        self.lib.rwkv_free(self.h)


def stats(v):
    return dict(median=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--model", default="7B")
    ap.add_argument("--widths", default="4,8,16")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rotations", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    widths = [int(x) for x in args.widths.split(",")]
    L, D = mf.SHAPES[args.model]
    max_ctx = max(widths) + 1                                    # the spare slot of leg (C)
    engine.lib()
    t = mf.synthetic_tensors_torch(L, D, seed=0)
    m = engine.RWKV(resident=True)
    m.loadTensors(L, D, t, maxGPT=max_ctx)
    parent = Parent(os.path.abspath(args.parent_lib), L, D, t, max_ctx)
    del t
    torch.cuda.empty_cache()
    line = dict(tool="beam_bench", model=args.model, n_layers=L, n_embed=D, steps=args.steps, reps=args.reps, rotations=args.rotations, maxGPT=max_ctx,
                device=torch.cuda.get_device_name(0), results={})
    text = []
    for W in widths:
        first = [int(v) for v in np.random.default_rng(W).integers(1, mf.VOCAB, W)]
        rot = [(s + 1) % W for s in range(W)]

        def timed(fn, per):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3 / per

        def leg_a():
            parent.chk(parent.lib.rwkv_reset_state(parent.h))
            return timed(lambda: parent.logprobs(first, args.steps, W + 1), args.steps)

        def leg_b():
            m.reset_state()
            return timed(lambda: m.decode_beam(first[0], args.steps, W), args.steps)

        def leg_c():
            return timed(lambda: [parent.rotate(W) for _ in range(args.rotations)], args.rotations)

        def leg_d():
            return timed(lambda: [m.state_permute(rot) for _ in range(args.rotations)], args.rotations)

        legs = dict(parent_logprobs=leg_a, beam=leg_b, parent_copies=leg_c, permute=leg_d)
        for fn in legs.values():                                 # warm every shape of the timed window
            fn()
        got = {k: [] for k in legs}
        for _ in range(args.reps):
            for k, fn in legs.items():
                got[k].append(fn())
        r = {k: stats(v) for k, v in got.items()}
        spread = lambda a, b: round(max(max(got[a]) - min(got[a]), max(got[b]) - min(got[b])), 4)
        moved = 40 * W * L * D                                   # bytes of W slots: read and written once into staging, once back
        r["select_and_gather_added_ms_per_step"] = round(r["beam"]["median"] - r["parent_logprobs"]["median"], 4)
        r["step_spread_ms"] = spread("parent_logprobs", "beam")
        r["permute_vs_copies_ms"] = round(r["permute"]["median"] - r["parent_copies"]["median"], 4)
        r["rotation_spread_ms"] = spread("parent_copies", "permute")
        r["rotation_bytes_each_way"] = moved
        r["permute_GB_per_s_read_plus_written"] = round(4 * moved / (r["permute"]["median"] * 1e-3) / 1e9, 1)
        line["results"][str(W)] = r
        msg = (f"W={W}: step parent_logprobs {r['parent_logprobs']['median']:.3f} ms ({r['parent_logprobs']['min']:.3f} .. {r['parent_logprobs']['max']:.3f}), "
               f"beam {r['beam']['median']:.3f} ms ({r['beam']['min']:.3f} .. {r['beam']['max']:.3f}), added {r['select_and_gather_added_ms_per_step']:+.3f} ms, "
               f"spread {r['step_spread_ms']:.3f} ms | rotation parent_copies {r['parent_copies']['median']:.3f} ms ({r['parent_copies']['min']:.3f} .. "
               f"{r['parent_copies']['max']:.3f}), permute {r['permute']['median']:.3f} ms ({r['permute']['min']:.3f} .. {r['permute']['max']:.3f}), "
               f"spread {r['rotation_spread_ms']:.3f} ms, {r['permute_GB_per_s_read_plus_written']} GB/s over {4 * moved / 1e6:.1f} MB")
        text.append(msg)
        print("[beam_bench] " + msg, file=sys.stderr, flush=True)
    line["resident_bytes"] = m.resident_bytes()
    parent.close()
    m.close()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "beam_bench.json"), "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")
        with open(os.path.join(args.out, "beam_bench.txt"), "w") as f:
            f.write("\n".join(text) + "\n")
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
