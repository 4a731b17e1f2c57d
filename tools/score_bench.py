#!/usr/bin/env python3
"""Scoring a prompt at 7B shapes: rwkv_score against the only way there was before it.

    python tools/score_bench.py [--model 7B] [--tokens 512] [--reps 8] [--warmup 2]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/score_bench.py --kernels-only
    python tools/score_bench.py --summarise OUT/.../*_kernel_stats.csv

Synthetic weights, maxGPT = --tokens, the state reset before every call, wall time around calls that are synchronous on return:
  (a) forward        rwkv_forward(tokens, GPT) alone: the prompt on the device
  (b) host_softmax   (a) + rwkv_get_output of the [tokens][50277] f32 logits + a numpy f64 log-softmax, entropy and argmax per row: what
                     a caller had to do
  (c) score          rwkv_score(tokens, targets): rows reduced on the device, 24 bytes per position downloaded
One JSON line on stdout.  --kernels-only runs (c) alone, for a kernel trace of its own (tracing slows the host: no wall times from that run);
--summarise reads the trace's kernel statistics and prints the device time of k_score_* next to that of every kernel of the run."""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summarise(path):
    rows = list(csv.DictReader(open(path)))
    tot = sum(int(r["TotalDurationNs"]) for r in rows)
    sc = [r for r in rows if "k_score_" in r["Name"]]
    out = dict(tool="score_bench", source=os.path.basename(path), all_kernels_ns=tot,
               score_kernels={r["Name"].split("(")[0].split("::")[-1]: dict(calls=int(r["Calls"]), total_ns=int(r["TotalDurationNs"]), average_ns=float(r["AverageNs"]))
                              for r in sc})
    out["score_kernels_ns"] = sum(int(r["TotalDurationNs"]) for r in sc)
    out["score_share_of_device_time"] = round(out["score_kernels_ns"] / tot, 6) if tot else None
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="7B")
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--summarise")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)

    import numpy as np
    import torch

    from rwkv_cpp_accelerated_amd import engine, modelfile as mf

    L, D = mf.SHAPES[args.model]
    n, V = args.tokens, mf.VOCAB
    lib = engine.lib()
    t = mf.synthetic_tensors_torch(L, D, seed=0)
    m = engine.RWKV(resident=True)
    m.loadTensors(L, D, t, maxGPT=n)
    del t
    torch.cuda.empty_cache()
    rng = np.random.default_rng(0)
    tokens = (C.c_uint64 * n)(*[int(v) for v in rng.integers(1, V, n)])
    targets = (C.c_uint64 * n)(*[int(v) for v in rng.integers(1, V, n)])
    tg = np.array(list(targets), np.int64)
    logits = np.zeros(n * V, np.float32)
    lp, ent, am = (C.c_double * n)(), (C.c_double * n)(), (C.c_uint64 * n)()
    host = {}

    def chk(rc):
        if rc != 0:
            raise RuntimeError(lib.rwkv_last_error().decode())

    def forward():
        chk(lib.rwkv_forward(m._h, tokens, n, engine.MODE_GPT))

    def host_softmax():
        forward()
        chk(lib.rwkv_get_output(m._h, C.c_void_p(logits.ctypes.data), None, None, None, None, None, n))
        l = logits.reshape(n, V).astype(np.float64)
        d = l - l.max(axis=1, keepdims=True)
        e = np.exp(d)
        z = e.sum(axis=1)
        host["lp"] = d[np.arange(n), tg] - np.log(z)
        host["ent"] = np.log(z) - (e * d).sum(axis=1) / z
        host["am"] = l.argmax(axis=1)

    def score():
        chk(lib.rwkv_score(m._h, tokens, targets, n, lp, ent, am))

    def timed(fn):
        for _ in range(args.warmup):
            m.reset_state(); fn()
        ts = []
        for _ in range(args.reps):
            m.reset_state()
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return ts

    if args.kernels_only:
        timed(score)
        m.close()
        return
    r = {k: timed(f) for k, f in (("forward", forward), ("host_softmax", host_softmax), ("score", score), ("forward_again", forward))}
    line = dict(tool="score_bench", model=args.model, n_layers=L, n_embed=D, tokens=n, maxGPT=n, reps=args.reps, device=torch.cuda.get_device_name(0),
                ms={k: dict(median=round(float(np.median(v)) * 1e3, 3), min=round(min(v) * 1e3, 3), max=round(max(v) * 1e3, 3)) for k, v in r.items()})
    f = float(np.median(r["forward"]))
    line["over_forward_ms"] = {k: round((float(np.median(r[k])) - f) * 1e3, 3) for k in ("host_softmax", "score")}
    line["download_bytes"] = dict(host_softmax=n * V * 4, score=n * 24)
    line["max_abs_diff_vs_host"] = dict(logprob=float(np.abs(np.array(list(lp)) - host["lp"]).max()), entropy=float(np.abs(np.array(list(ent)) - host["ent"]).max()),
                                        argmax_equal=bool(np.array_equal(np.array(list(am), np.int64), host["am"])))
    line["resident_bytes"] = m.resident_bytes()
    m.close()
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
