#!/usr/bin/env python3
"""Speculative sampling with a draft model that samples, at 7B shapes: what the ratio pick and the stash cost.

    python tools/spec_ratio_bench.py [--model 7B] [--draft 169M] [--n-drafts 3,7,31] [--ks 4,8] [--reps 5] [--iters 8] [--tokens 96]
                                     [--out profiles/spec_ratio]

  verify   per n_draft, alternating: rwkv_spec_verify (the greedy pick: two argmax launches) against rwkv_spec_verify_ratio (one k_ratio_pick
           launch over n_draft + 1 rows, q_logits = rows of the draft context's logits buffer); the same pass, accept and commit in both.  A draft
           of random ids is rejected at row 0 by either, which is the ratio pick's expensive side: every row runs all three sweeps.
  loop     per k, alternating: rwkv_decode_speculative (greedy draft, greedy pick; its kernels are the parent commit's, isa_compare.txt) against
           rwkv_decode_speculative_sampled with the --draft shaped model of another seed; ms per round.  The difference is the draft's sampler in
           place of the argmax node of its token graph, the stash copies and the ratio pick.
--reps rounds of the two legs in turn after a warm round; median and min .. max; `spread` is the larger max - min of the two legs.
Wall clock around synchronous calls.  Synthetic weights: acceptance on real text is NOT measured here (a draft of another seed is rejected
almost always, so a round emits one id: the worst case's round)."""
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


def stats(v):
    return dict(median=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4))


def fmt(s):
    return f"{s['median']:.3f} ms ({s['min']:.3f} .. {s['max']:.3f})"


def timed(fn, per=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3 / per


def alternate(legs, reps, say, what):
    """legs: name -> fn returning ms; one warm round, then `reps` rounds in turn"""
    for fn in legs.values():
        fn()
    got = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            got[k].append(fn())
    r = {k: stats(v) for k, v in got.items()}
    a, b = list(legs)
    r["added_ms"] = round(r[b]["median"] - r[a]["median"], 4)
    r["spread_ms"] = round(max(max(v) - min(v) for v in got.values()), 4)
    say(f"{what}: {a} {fmt(r[a])}, {b} {fmt(r[b])}, added {r['added_ms']:+.3f} ms, spread {r['spread_ms']:.3f} ms")
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="7B")
    ap.add_argument("--draft", default="169M")
    ap.add_argument("--n-drafts", default="3,7,31")
    ap.add_argument("--ks", default="4,8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--tokens", type=int, default=96)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L, D = mf.SHAPES[args.model]
    Ld, Dd = mf.SHAPES[args.draft]
    max_ctx = 34
    engine.lib()
    m, small = engine.RWKV(resident=True), engine.RWKV(resident=True)
    m.loadTensors(L, D, mf.synthetic_tensors_torch(L, D, seed=0), maxGPT=max_ctx)
    small.loadTensors(Ld, Dd, mf.synthetic_tensors_torch(Ld, Dd, seed=1), maxGPT=max_ctx)
    torch.cuda.empty_cache()
    line = dict(tool="spec_ratio_bench", model=args.model, draft=args.draft, reps=args.reps, iters=args.iters, tokens=args.tokens,
                device=torch.cuda.get_device_name(0), verify={}, loop={})
    text = []

    def say(msg):
        text.append(msg)
        print("[spec_ratio_bench] " + msg, file=sys.stderr, flush=True)

    rng = np.random.default_rng(3)
    small.forward([int(v) for v in rng.integers(2, mf.VOCAB, max_ctx)], engine.MODE_PARRALEL)      # 34 rows of draft logits to judge against
    for nd in [int(x) for x in args.n_drafts.split(",")]:
        rows = [int(v) for v in rng.integers(2, mf.VOCAB, nd + 1)]
        line["verify"][str(nd)] = alternate(dict(
            verify=lambda: timed(lambda: [m.spec_verify(rows[0], rows[1:]) for _ in range(args.iters)], args.iters),
            verify_ratio=lambda: timed(lambda: [m.spec_verify_ratio(rows[0], rows[1:], small, 7, 0, 0.8, 1.0) for _ in range(args.iters)], args.iters),
        ), args.reps, say, f"n_draft={nd}")

    prompt = [int(v) for v in np.random.default_rng(5).integers(2, mf.VOCAB, 8)]

    def loop(fn):
        for x in (m, small):
            x.reset_state()
            x.forward(prompt, engine.MODE_GPT)
        t0 = time.perf_counter()
        _, st = fn()
        loop.last = st
        return (time.perf_counter() - t0) * 1e3 / st["rounds"]

    for k in [int(x) for x in args.ks.split(",")]:
        r = alternate(dict(greedy=lambda: loop(lambda: m.decode_speculative(small, 5, args.tokens, k)),
                           sampled=lambda: loop(lambda: m.decode_speculative_sampled(small, 5, args.tokens, k, 0.8, 1.0, 7, 9))),
                      args.reps, say, f"k={k}, ms per round")
        r["sampled_stats"] = loop.last
        line["loop"][str(k)] = r
    line["resident_bytes"] = dict(target=m.resident_bytes(), draft=small.resident_bytes())
    for x in (m, small):
        x.close()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "spec_ratio_bench.json"), "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")
        with open(os.path.join(args.out, "spec_ratio_bench.txt"), "w") as f:
            f.write("\n".join(text) + "\n")
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
