#!/usr/bin/env python3
"""What a min-p or Mirostat pick costs per step in the device decode loop, next to the nucleus pick and to the host loop they replace.

    python tools/floor_bench.py [--model 7B] [--streams 1,32,96] [--steps 32] [--reps 5] [--out profiles/floor]

One context at --model shapes, one process.  Per stream count N the legs run in turn, --reps rounds behind a warm round, each leg one
decode_batch_until call of --steps steps from the same state:
  greedy     the loop without a sampler: the baseline every other leg is charged against
  nucleus    temp 1, top_p 0.9, top_k 40, penalties: three launches and 1.84 MB of scratch per row (unchanged by this work)
  minp       temp 1, min_p 0.05, penalties: two launches, no per-token scratch (csrc/floor.hip.h)
  mirostat   temp 1, tau 5, eta 0.1, penalties: the same two launches with the tempered sum
  host       what a caller without these kinds runs: forward, download of N x 201 KB logits, a numpy min-p pick per stream, upload of the ids
ms per step: median (min .. max) over the rounds; `over greedy` = median - greedy's median; `spread` is the largest max - min among the legs of
a line: a difference inside it is not a difference.  Wall clock around synchronous calls."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from rwkv_cpp_accelerated_amd import engine, modelfile as mf

PEN = dict(presence=0.4, frequency=0.4, decay=0.996)
PICKS = dict(greedy=dict(pick="greedy"), nucleus=dict(pick="nucleus", temp=1.0, top_p=0.9, top_k=40, **PEN),
             minp=dict(pick="minp", temp=1.0, min_p=0.05, **PEN), mirostat=dict(pick="mirostat", temp=1.0, tau=5.0, eta=0.1, **PEN))


def host_step(m, ids, rng):
    """one step of the loop the device kinds replace: forward, logits download, min-p 0.05 per stream in numpy"""
    n = len(ids)
    lg = m.forward(ids, engine.MODE_PARRALEL)[: n * mf.VOCAB].reshape(n, mf.VOCAB).astype(np.float64)
    lg[:, 0] = -99.0
    out = []
    for row in lg:
        w = np.where(row - row.max() >= np.log(0.05), np.exp(row - row.max()), 0.0)
        c = np.cumsum(w)
        out.append(int(min(np.searchsorted(c, rng.random() * c[-1], side="right"), mf.VOCAB - 1)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="7B")
    ap.add_argument("--streams", default="1,32,96")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    streams = [int(v) for v in args.streams.split(",")]
    L, D = mf.SHAPES[args.model]
    m = engine.RWKV(resident=True)
    m.loadTensors(L, D, mf.synthetic_tensors_torch(L, D, seed=0), maxGPT=max(streams))
    rng = np.random.default_rng(1)
    line = dict(tool="floor_bench", model=args.model, steps=args.steps, reps=args.reps, device=torch.cuda.get_device_name(0), streams={})
    text = []
    for n in streams:
        first = [int(v) for v in rng.integers(1, mf.VOCAB, n)]
        legs = {k: (lambda kw=kw: m.decode_batch_until(first, args.steps, seeds=list(range(n)), **kw)) for k, kw in PICKS.items()}

        def host():
            ids = list(first)
            for _ in range(args.steps):
                ids = host_step(m, ids, rng)
        legs["host"] = host
        got = {k: [] for k in legs}
        for r in range(args.reps + 1):
            for k, fn in legs.items():
                m.reset_state()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                if r:
                    got[k].append((time.perf_counter() - t0) * 1e3 / args.steps)
        res = {k: dict(median=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4)) for k, v in got.items()}
        spread = round(max(s["max"] - s["min"] for k, s in res.items() if k != "host"), 4)
        for k, s in res.items():
            s["over_greedy"] = round(s["median"] - res["greedy"]["median"], 4)
        line["streams"][str(n)] = dict(legs=res, spread=spread)
        msg = f"N {n:3d}: " + "; ".join(f"{k} {s['median']:.3f} ms ({s['min']:.3f} .. {s['max']:.3f}) +{s['over_greedy']:.3f}" for k, s in res.items()) + f"; spread {spread:.3f} ms"
        text.append(msg)
        print("[floor_bench] " + msg, file=sys.stderr, flush=True)
    m.close()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "floor_bench.json"), "w") as f:
            json.dump(line, f, indent=1)
        with open(os.path.join(args.out, "floor_bench.txt"), "w") as f:
            f.write("\n".join(text) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
