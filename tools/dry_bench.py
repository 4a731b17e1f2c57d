#!/usr/bin/env python3
"""What the DRY penalty costs per step at 7B shapes (rwkv_decode_batch_dry, csrc/dry.hip.h).

    python tools/dry_bench.py [--model 7B] [--streams 1,32,96] [--steps 64] [--reps 5] [--rounds 2] [--parent-tree DIR]

Per N streams, greedy, synthetic weights, every call from the zero state and from freshly planted histories:
  constrained    rwkv_decode_batch_constrained without an automaton, a three-entry bias list per stream: the call a DRY call is built on
  dry_H_hits     rwkv_decode_batch_dry with the same arguments, multiplier 0.8, base 1.75, allowed_length 2, window 4096, over planted histories
                 of H = 256 / 4096 ids that hold the first token 0 or 64 times (the hits of step 0; later steps search what the stream writes)
  host           the loop it replaces: per step rwkv_forward, rwkv_get_output of the N logits rows, a numpy scan of the history, the
                 subtraction and numpy's argmax (--host-steps steps, history 4096, 64 hits)
One process loads the model once and runs `reps` repetitions with the variants interleaved.  The orchestrator starts `rounds` such processes one
after the other; with --parent-tree (a checkout of the parent commit with its engine built) the rounds alternate with a process that times
`constrained` with that tree's package and library.  Per figure: the median over all repetitions of all rounds and min .. max; per difference
the run-to-run spread of the two figures it is taken from.  One JSON line on stdout."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRY = dict(multiplier=0.8, base=1.75, allowed_length=2, window=4096)


def history(np, V, H, hits, first, seed):
    """H distinct ids above 25000 (none is `first`, which is below), `first` planted at `hits` places"""
    h = np.random.default_rng(seed).permutation(np.arange(25000, V))[:H].astype(np.int64)
    if hits:
        h[np.linspace(1, H - 2, hits).astype(int)] = first
    return h.tolist()


def host_scan(np, h, allowed):
    """{id: L} over the history (the header's scan), numpy for the hit search"""
    h = np.asarray(h[-DRY["window"]:])
    best = {}
    for j in np.flatnonzero(h[:-1] == h[-1]):
        m = 0
        while m < 64 and j - m >= 0 and h[j - m] == h[len(h) - 1 - m]:
            m += 1
        best[int(h[j + 1])] = max(best.get(int(h[j + 1]), 0), m)
    return {t: l for t, l in best.items() if l >= allowed}


def child(args):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.abspath(args.tree or ROOT))
    from rwkv_cpp_accelerated_amd import engine, modelfile as mf
    ns = [int(x) for x in args.streams.split(",")]
    L, D = mf.SHAPES[args.model]
    lib, V, full = engine.lib(), mf.VOCAB, args.child == "all"
    m = engine.RWKV(resident=True)
    m.loadTensors(L, D, mf.synthetic_tensors_torch(L, D, seed=0), maxGPT=max(ns))
    torch.cuda.empty_cache()
    out = dict(child=args.child, lib=engine.LIB_PATH, device=torch.cuda.get_device_name(0), results={})
    for n in ns:
        first = [int(v) for v in np.random.default_rng(n).integers(1, 25000, n)]
        bias = [{100 + s: 0.5, 200 + s: -0.5, 300 + s: 0.25} for s in range(n)]
        variants = {"constrained": (None, lambda k: m.decode_batch_constrained(first, k, bias=bias)[0])}
        if full:
            for H in (256, 4096):
                for hits in (0, 64):
                    variants[f"dry_{H}_{hits}"] = ([history(np, V, H, hits, first[s], 1000 * n + s) for s in range(n)],
                                                   lambda k: m.decode_batch_dry(first, k, bias=bias, **DRY)[0])

        def run(name, k):
            hist, fn = variants[name]
            for s in range(n if hist else 0):
                m.dry_history_set(hist[s], s)
            m.reset_state()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(k)                                   # synchronous: the call ends behind its download
            return (time.perf_counter() - t0) / k * 1e3

        for name in variants:
            run(name, args.steps)                   # warm every shape of the timed window
        ms = {name: [] for name in variants}
        for _ in range(args.reps):
            for name in variants:
                ms[name].append(round(run(name, args.steps), 4))
        if full:
            logits = np.zeros(n * V, np.float32)
            pen = [DRY["multiplier"] * DRY["base"] ** i for i in range(64)]

            def host(k):                            # the caller's loop the call replaces
                cur, hist = list(first), [list(h) for h in variants["dry_4096_64"][0]]
                for _ in range(k):
                    rc = lib.rwkv_forward(m._h, (C.c_uint64 * n)(*cur), n, engine.MODE_PARRALEL if n > 1 else engine.MODE_GPT)
                    rc = rc or lib.rwkv_get_output(m._h, C.c_void_p(logits.ctypes.data), None, None, None, None, None, n)
                    if rc:
                        raise RuntimeError(lib.rwkv_last_error().decode())
                    lg = logits.reshape(n, V)
                    for s in range(n):
                        hist[s].append(cur[s])
                        for t, l in host_scan(np, hist[s], DRY["allowed_length"]).items():
                            lg[s, t] -= pen[l - DRY["allowed_length"]]
                        cur[s] = 1 + int(np.argmax(lg[s, 1:]))
                return cur

            host(2)
            for _ in range(max(2, args.reps // 2)):
                m.reset_state(); torch.cuda.synchronize()
                t0 = time.perf_counter()
                host(args.host_steps)
                ms.setdefault("host", []).append(round((time.perf_counter() - t0) / args.host_steps * 1e3, 4))
        out["results"][str(n)] = ms
        print(f"[dry_bench:{args.child}] N={n}: " + ", ".join(f"{k} {np.median(v):.3f}" for k, v in ms.items()) + " ms/step", file=sys.stderr, flush=True)
    m.close()
    print(json.dumps(out), flush=True)


def stats(v):
    import numpy as np
    return dict(median=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4), n=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="7B")
    ap.add_argument("--streams", default="1,32,96")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--host-steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: `constrained` is timed on it too")
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child", default=None, choices=["all", "constrained"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    base = [sys.executable, os.path.abspath(__file__), "--model", args.model, "--streams", args.streams, "--steps", str(args.steps),
            "--host-steps", str(args.host_steps), "--reps", str(args.reps)]
    pooled, device = {}, None

    def run(kind, tree):                            # a fresh process per measurement: its own context, its own package and library
        nonlocal device
        p = subprocess.run(base + ["--child", kind] + (["--tree", tree] if tree else []), stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"the {kind} process failed with status {p.returncode}")
        r = json.loads(p.stdout.strip().splitlines()[-1])
        device = r["device"]
        for case, ms in r["results"].items():
            for name, v in ms.items():
                pooled.setdefault(case, {}).setdefault(("parent_" if tree else "") + name, []).extend(v)

    for _ in range(args.rounds):
        if args.parent_tree:
            run("constrained", args.parent_tree)
        run("all", None)
    line = dict(tool="dry_bench", model=args.model, steps=args.steps, host_steps=args.host_steps, reps=args.reps, rounds=args.rounds, device=device,
                unit="ms per step", dry=DRY, results={})
    for case, ms in pooled.items():
        r = {name: stats(v) for name, v in ms.items()}
        ref = "parent_constrained" if "parent_constrained" in r else "constrained"
        spread = lambda a, b: round(max(r[a]["max"] - r[a]["min"], r[b]["max"] - r[b]["min"]) * 1e3, 1)
        r[f"added_us_per_step_over_{ref}"] = {name: dict(added=round((r[name]["median"] - r[ref]["median"]) * 1e3, 1), spread=spread(name, ref))
                                              for name in r if name.startswith("dry_") or (name == "constrained" and ref != name)}
        line["results"]["N=" + case] = r
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
