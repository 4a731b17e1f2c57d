#!/usr/bin/env python3
"""What the log-prob record costs per step at 7B shapes (rwkv_decode_batch_logprobs, csrc/topn.hip.h).

    python tools/logprobs_bench.py [--model 7B] [--streams 1,32,96] [--steps 64] [--reps 5] [--rounds 2] [--parent-tree DIR]

Per N streams and pick (greedy; nucleus with top_p 0.9, top_k 40 and penalties), synthetic weights, every call from the zero state:
  until        rwkv_decode_batch_until with a stop sequence that never matches and budgets equal to steps (the stop hooks run, nothing stops)
  logprobs_n   rwkv_decode_batch_logprobs with the same arguments and top_n = 0, 5, 20, 32: the same picks (checked) plus the record
  host         what the record replaces: one call of one step at a time, rwkv_get_output of the N logits rows and a numpy f64 log-softmax and
               top-20 per row (greedy picks, --host-steps steps)
One process loads the model once and runs `reps` repetitions with the variants interleaved (until, logprobs_0, ..., until, ...), so a
difference between two variants is taken inside one process on one GPU.  The orchestrator starts `rounds` such processes one after the
other; with --parent-tree (a checkout of the parent commit with its engine built) each round first runs a process that times `until` with
that tree's package and library, which shows what this change costs a call that does not ask for the record.  Per figure: the median over all
repetitions of all rounds and min .. max; per difference: the run-to-run spread of the two figures it is taken from next to it.
One JSON line on stdout."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NUC = dict(temp=1.0, top_p=0.9, top_k=40, presence=0.4, frequency=0.4, decay=0.996)
TOP_NS = (0, 5, 20, 32)
HOST_TOPN = 20


def child(args):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.abspath(args.tree or ROOT))
    from rwkv_cpp_accelerated_amd import engine, modelfile as mf
    ns = [int(x) for x in args.streams.split(",")]
    L, D = mf.SHAPES[args.model]
    lib = engine.lib()
    has_lp = args.child == "all"
    t = mf.synthetic_tensors_torch(L, D, seed=0)
    m = engine.RWKV(resident=True)
    m.loadTensors(L, D, t, maxGPT=max(ns))
    del t
    torch.cuda.empty_cache()
    V = mf.VOCAB
    out = dict(child=args.child, lib=engine.LIB_PATH, device=torch.cuda.get_device_name(0), results={})
    for n in ns:
        first = [int(v) for v in np.random.default_rng(n).integers(1, V, n)]
        seeds = list(range(n))
        never = [[V - 1] * 8]
        for pick in ("greedy", "nucleus"):
            kw = dict(pick=pick, seeds=seeds, stops=never, **(NUC if pick == "nucleus" else {}))
            variants = {"until": lambda k: m.decode_batch_until(first, k, max_new=[k] * n, **kw)[0]}
            if has_lp:
                for tn in TOP_NS:
                    variants[f"logprobs_{tn}"] = lambda k, tn=tn: m.decode_batch_logprobs(first, k, top_n=tn, max_new=[k] * n, **kw)[0]

            def timed(fn, k):
                m.reset_state()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ids = fn(k)                         # synchronous: the call ends behind its download
                return (time.perf_counter() - t0) / k * 1e3, ids

            ref = None
            for fn in variants.values():            # warm every shape of the timed window; the picks do not depend on the record
                m.reset_state()
                ids = fn(args.steps)
                ref = ids if ref is None else ref
                assert np.array_equal(ids, ref), "the record changed the picks"
            ms = {name: [] for name in variants}
            for _ in range(args.reps):
                for name, fn in variants.items():
                    ms[name].append(round(timed(fn, args.steps)[0], 4))
            out["results"][f"{n}/{pick}"] = ms
            print(f"[logprobs_bench:{args.child}] N={n} {pick}: " + ", ".join(f"{k} {np.median(v):.3f}" for k, v in ms.items()) + " ms/step",
                  file=sys.stderr, flush=True)
        if not has_lp:
            continue
        logits = np.zeros(n * V, np.float32)

        def host(k):                                # the caller's loop the record replaces
            cur, total = list(first), 0.0
            for _ in range(k):
                rc = lib.rwkv_forward(m._h, (C.c_uint64 * n)(*cur), n, engine.MODE_PARRALEL)
                rc = rc or lib.rwkv_get_output(m._h, C.c_void_p(logits.ctypes.data), None, None, None, None, None, n)
                if rc:
                    raise RuntimeError(lib.rwkv_last_error().decode())
                lg = logits.reshape(n, V).astype(np.float64)
                lse = np.log(np.exp(lg - lg.max(axis=1, keepdims=True)).sum(axis=1)) + lg.max(axis=1)
                top = np.argpartition(-lg, HOST_TOPN, axis=1)[:, :HOST_TOPN]
                top = np.take_along_axis(top, np.argsort(-np.take_along_axis(lg, top, axis=1), axis=1, kind="stable"), axis=1)
                total += float((np.take_along_axis(lg, top, axis=1) - lse[:, None]).sum())
                lg[:, 0] = -np.inf
                cur = [int(x) for x in lg.argmax(axis=1)]
            return total

        host(2)
        hs = []
        for _ in range(max(2, args.reps // 2)):
            m.reset_state(); torch.cuda.synchronize()
            t0 = time.perf_counter()
            host(args.host_steps)
            hs.append(round((time.perf_counter() - t0) / args.host_steps * 1e3, 4))
        out["results"][f"{n}/host_top{HOST_TOPN}"] = dict(host=hs)
        print(f"[logprobs_bench:{args.child}] N={n} host loop: {np.median(hs):.3f} ms/step", file=sys.stderr, flush=True)
    out["resident_bytes"] = m.resident_bytes()
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
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: `until` is timed on it too")
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child", default=None, choices=["all", "until"], help=argparse.SUPPRESS)
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
            run("until", args.parent_tree)
        run("all", None)
    line = dict(tool="logprobs_bench", model=args.model, steps=args.steps, host_steps=args.host_steps, reps=args.reps, rounds=args.rounds,
                device=device, unit="ms per step", results={})
    for case, ms in pooled.items():
        r = {name: stats(v) for name, v in ms.items()}
        if "until" in r:
            spread = lambda a, b: round(max(r[a]["max"] - r[a]["min"], r[b]["max"] - r[b]["min"]) * 1e3, 1)
            r["added_us_per_step"] = {name: dict(added=round((r[name]["median"] - r["until"]["median"]) * 1e3, 1), spread=spread(name, "until"))
                                      for name in r if name.startswith("logprobs_")}
            if "parent_until" in r:
                r["until_vs_parent_us_per_step"] = dict(added=round((r["until"]["median"] - r["parent_until"]["median"]) * 1e3, 1),
                                                        spread=spread("until", "parent_until"))
        line["results"][case] = r
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
