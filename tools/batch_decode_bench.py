#!/usr/bin/env python3
"""Batched decode at 7B shapes: what N streams cost per step when the caller generates text with them.

    python tools/batch_decode_bench.py [--model 7B] [--streams 32,64,96] [--steps 24] [--warmup 4]

Per N (synthetic weights, state slots 0 .. N - 1, maxGPT = the largest N):
  (a) bare_step      rwkv_forward(N tokens, PARRALEL) alone -- the GPU step, ids fixed
  (b) host_loop      (a) + rwkv_get_output of the N logits rows + numpy argmax (logit 0 banned) + the next ids: what a caller without
                     the batched entry points has to do
  (c) batch_greedy   rwkv_decode_batch_greedy(N, steps): picks on the device, one upload and one download per call
  (d) batch_typical  rwkv_decode_batch_typical(N, steps), default mode and RWKV_SAMPLE_RECIPE
  (e) batch_nucleus  rwkv_decode_batch_nucleus(N, steps): top_p 0.9 alone, and the full form (top_p 0.9, top_k 40, penalties 0.4 / 0.4, decay 0.996)
ms per step and aggregate tokens/s (N / step time), one JSON line on stdout.

    python tools/batch_decode_bench.py --until [--streams 1,32,96] [--steps 64] [--reps 5]

What stopping costs (rwkv_decode_batch_until): per N, interleaved A / B over --reps rounds,
  (A) plain          rwkv_decode_batch_nucleus(N, steps), the full form (N = 1: the decode kernels, as rwkv_decode_nucleus)
  (B) until          the same picks through rwkv_decode_batch_until with a stop sequence that never matches and budgets equal to steps:
                     the stop test and the park launch behind every step, the poll every 8 steps, nothing parked
median and min .. max of ms per step of each, and the added microseconds per step; then one call of 4096 steps whose streams all stop at
step 20 -- its steps_run and wall time -- next to the same 20 tokens made one call of one step at a time (the host's loop)."""
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


NUC = dict(temp=1.0, top_p=0.9, top_k=40, presence=0.4, frequency=0.4, decay=0.996)      # the full form of (e)


def until_bench(m, args, ns, line):
    V = mf.VOCAB
    for n in ns:
        first = [int(v) for v in np.random.default_rng(n).integers(1, V, n)]
        seeds = list(range(n))
        never = [[V - 1] * 8]                       # eight times the last id in a row: not what a synthetic model says

        def plain(k):
            return m.decode_batch_nucleus(first, k, seeds=seeds, **NUC)

        def until(k, stops=never, max_new=None):
            return m.decode_batch_until(first, k, stops=stops, max_new=[k] * n if max_new is None else max_new, pick="nucleus", seeds=seeds, **NUC)

        def timed(fn, k):
            m.reset_state()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(k)
            return (time.perf_counter() - t0) / k, out

        for fn in (plain, until):                   # warm every shape of the timed window
            fn(args.steps)
        a, b = [], []
        for _ in range(args.reps):
            ta, ids_a = timed(plain, args.steps)
            tb, (ids_b, ln, rs, ran) = timed(until, args.steps)
            assert np.array_equal(ids_a, ids_b) and ran == args.steps and not rs.any(), "the never-matching sequence matched"
            a.append(ta * 1e3); b.append(tb * 1e3)
        long, stop_at = 4096, 20
        until(long, stops=[], max_new=[stop_at] * n)
        m.reset_state(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        ids, ln, rs, ran = until(long, stops=[], max_new=[stop_at] * n)
        t_until = time.perf_counter() - t0
        assert ln.tolist() == [stop_at] * n
        m.reset_state(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        cur = list(first)
        for k in range(stop_at):                    # the host's loop: one token per call, one round trip each
            cur = [int(v) for v in m.decode_batch_nucleus(cur, 1, seeds=[s + k for s in seeds], keep=k > 0, **NUC)[:, 0]]
        t_host = time.perf_counter() - t0
        assert cur == [int(v) for v in ids[:, stop_at - 1]]
        r = dict(plain_ms_per_step=dict(median=round(float(np.median(a)), 4), min=round(min(a), 4), max=round(max(a), 4)),
                 until_ms_per_step=dict(median=round(float(np.median(b)), 4), min=round(min(b), 4), max=round(max(b), 4)),
                 added_us_per_step=round((float(np.median(b)) - float(np.median(a))) * 1e3, 2),
                 spread_us=round(max(max(a) - min(a), max(b) - min(b)) * 1e3, 2),
                 stop_at_20_of_4096=dict(steps_run=int(ran), until_ms=round(t_until * 1e3, 3), host_one_token_per_call_ms=round(t_host * 1e3, 3)))
        line["results"][str(n)] = r
        print(f"[batch_decode_bench] until N={n}: {json.dumps(r)}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="7B")
    ap.add_argument("--streams", default=None)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--until", action="store_true", help="measure rwkv_decode_batch_until against the plain nucleus loop")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    args.streams = args.streams or ("1,32,96" if args.until else "32,64,96")
    args.steps = args.steps or (64 if args.until else 24)
    ns = [int(x) for x in args.streams.split(",")]
    L, D = mf.SHAPES[args.model]
    lib = engine.lib()
    t = mf.synthetic_tensors_torch(L, D, seed=0)
    m = engine.RWKV(resident=True)
    m.loadTensors(L, D, t, maxGPT=max(ns))
    del t
    torch.cuda.empty_cache()
    V = mf.VOCAB
    line = dict(tool="batch_decode_bench", model=args.model, n_layers=L, n_embed=D, steps=args.steps, maxGPT=max(ns),
                device=torch.cuda.get_device_name(0), results={})

    def chk(rc):
        if rc != 0:
            raise RuntimeError(lib.rwkv_last_error().decode())

    if args.until:
        line["mode"] = "until"
        line["reps"] = args.reps
        until_bench(m, args, ns, line)
        ns = []
    for n in ns:
        rng = np.random.default_rng(n)
        first = [int(v) for v in rng.integers(1, V, n)]
        ids = (C.c_uint64 * n)(*first)
        logits = np.zeros(n * V, np.float32)

        def bare(k):
            for _ in range(k):
                chk(lib.rwkv_forward(m._h, ids, n, engine.MODE_PARRALEL))

        def host(k):
            cur = list(first)
            for _ in range(k):
                chk(lib.rwkv_forward(m._h, (C.c_uint64 * n)(*cur), n, engine.MODE_PARRALEL))
                chk(lib.rwkv_get_output(m._h, C.c_void_p(logits.ctypes.data), None, None, None, None, None, n))
                lg = logits.reshape(n, V)
                lg[:, 0] = -np.inf
                cur = [int(x) for x in lg.argmax(axis=1)]

        def timed(fn, k):
            m.reset_state()
            fn(args.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(k)
            return (time.perf_counter() - t0) / k

        r = {}
        r["bare_step"] = timed(bare, args.steps)
        r["host_loop"] = timed(host, args.steps)
        r["batch_greedy"] = timed(lambda k: m.decode_batch_greedy(first, k), args.steps)
        r["batch_typical"] = timed(lambda k: m.decode_batch_typical(first, k, seeds=list(range(n))), args.steps)
        r["batch_typical_recipe"] = timed(lambda k: m.decode_batch_typical(first, k, seeds=list(range(n)), recipe=True), args.steps)
        r["batch_nucleus"] = timed(lambda k: m.decode_batch_nucleus(first, k, temp=1.0, top_p=0.9, seeds=list(range(n))), args.steps)
        r["batch_nucleus_full"] = timed(lambda k: m.decode_batch_nucleus(first, k, temp=1.0, top_p=0.9, top_k=40, presence=0.4, frequency=0.4,
                                                                         decay=0.996, seeds=list(range(n))), args.steps)
        out = {k: dict(ms_per_step=round(v * 1e3, 3), aggregate_tokens_per_s=round(n / v, 1)) for k, v in r.items()}
        b = r["bare_step"]
        out["vs_bare_step"] = {k: round(v / b - 1.0, 4) for k, v in r.items() if k != "bare_step"}
        line["results"][str(n)] = out
        print(f"[batch_decode_bench] N={n}: " + ", ".join(f"{k} {v * 1e3:.3f} ms" for k, v in r.items()), file=sys.stderr, flush=True)
    line["resident_bytes"] = m.resident_bytes()
    m.close()
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
