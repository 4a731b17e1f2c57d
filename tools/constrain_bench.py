#!/usr/bin/env python3
"""What constrained decoding costs per step at 7B shapes (rwkv_decode_batch_constrained, csrc/constrain.hip.h).

    python tools/constrain_bench.py [--model 7B] [--streams 1,32,96] [--steps 64] [--reps 5] [--rounds 2] [--parent-tree DIR]

Per N streams and pick (greedy; nucleus with top_p 0.9, top_k 40 and penalties), synthetic weights, every call from the zero state:
  until          rwkv_decode_batch_until with a stop sequence that never matches and budgets equal to steps (the stop hooks run, nothing stops)
  everything     rwkv_decode_batch_constrained with the same arguments under the allow-everything automaton (one state, 50276 self-loops): the
                 same picks (checked for greedy), plus k_constrain_rows and k_constraint_advance per step
  sparse         the same under a synthetic sparse automaton, 256 states x 64 edges, no terminal state
  sparse_bias    the same with a 300-entry bias list per stream
  host           the loop it replaces: per step rwkv_forward, rwkv_get_output of the N logits rows, a numpy mask, the upload of the rows into
                 the logits buffer and rwkv_sample_nucleus per row (--host-steps steps)
One process loads the model once and runs `reps` repetitions with the variants interleaved, so a difference between two variants is taken
inside one process on one GPU.  The orchestrator starts `rounds` such processes one after the other; with --parent-tree (a checkout of the
parent commit with its engine built) each round first runs a process that times `until` with that tree's package and library: what this change
costs a call that does not ask for a constraint.  Per figure: the median over all repetitions of all rounds and min .. max; per difference: the
run-to-run spread of the two figures it is taken from next to it.  One JSON line on stdout."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NUC = dict(temp=1.0, top_p=0.9, top_k=40, presence=0.4, frequency=0.4, decay=0.996)
SPARSE_STATES, SPARSE_EDGES, BIAS_N = 256, 64, 300


def automata(np, V):
    rng = np.random.default_rng(11)
    tok = np.concatenate([np.sort(rng.choice(np.arange(1, V), SPARSE_EDGES, replace=False)) for _ in range(SPARSE_STATES)]).astype(np.uint32)
    nxt = rng.integers(0, SPARSE_STATES, tok.size).astype(np.uint32)
    sparse = (np.arange(0, tok.size + 1, SPARSE_EDGES, dtype=np.uint32), tok, nxt)
    everything = (np.array([0, V - 1], np.uint32), np.arange(1, V, dtype=np.uint32), np.zeros(V - 1, np.uint32))
    return everything, sparse


def child(args):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.abspath(args.tree or ROOT))
    from rwkv_cpp_accelerated_amd import engine, modelfile as mf
    ns = [int(x) for x in args.streams.split(",")]
    L, D = mf.SHAPES[args.model]
    lib = engine.lib()
    full = args.child == "all"
    t = mf.synthetic_tensors_torch(L, D, seed=0)
    m = engine.RWKV(resident=True)
    m.loadTensors(L, D, t, maxGPT=max(ns))
    del t
    torch.cuda.empty_cache()
    V = mf.VOCAB
    everything, sparse = automata(np, V)
    out = dict(child=args.child, lib=engine.LIB_PATH, device=torch.cuda.get_device_name(0), results={})
    for n in ns:
        first = [int(v) for v in np.random.default_rng(n).integers(1, V, n)]
        seeds = list(range(n))
        never = [[V - 1] * 8]
        rng = np.random.default_rng(100 + n)
        bias = [{int(i): float(v) for i, v in zip(rng.choice(np.arange(1, V), BIAS_N, replace=False), rng.standard_normal(BIAS_N))} for _ in range(n)]
        for pick in ("greedy", "nucleus"):
            kw = dict(pick=pick, seeds=seeds, stops=never, **(NUC if pick == "nucleus" else {}))
            variants = {"until": (None, lambda k: m.decode_batch_until(first, k, max_new=[k] * n, **kw)[0])}
            if full:
                con = lambda k, b=None: m.decode_batch_constrained(first, k, start=[0] * n, bias=b, max_new=[k] * n, **kw)[0]
                variants["everything"] = (everything, con)
                variants["sparse"] = (sparse, con)
                variants["sparse_bias"] = (sparse, lambda k: con(k, bias))
            installed = [None]

            def run(name, k):
                a, fn = variants[name]
                if a is not None and installed[0] is not a:
                    m.constraint_set(*a)
                    installed[0] = a
                m.reset_state()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ids = fn(k)                         # synchronous: the call ends behind its download
                return (time.perf_counter() - t0) / k * 1e3, ids

            ref = run("until", args.steps)[1]       # warm every shape of the timed window
            for name in list(variants)[1:]:
                ids = run(name, args.steps)[1]
                if name == "everything" and pick == "greedy":
                    assert np.array_equal(ids, ref), "the allow-everything automaton changed the greedy picks"
            ms = {name: [] for name in variants}
            for _ in range(args.reps):
                for name in variants:
                    ms[name].append(round(run(name, args.steps)[0], 4))
            out["results"][f"{n}/{pick}"] = ms
            print(f"[constrain_bench:{args.child}] N={n} {pick}: " + ", ".join(f"{k} {np.median(v):.3f}" for k, v in ms.items()) + " ms/step",
                  file=sys.stderr, flush=True)
        if not full:
            continue
        m.constraint_clear()
        logits = np.zeros(n * V, np.float32)
        rp, tk, nx = sparse
        view = None
        try:                                        # the upload of the masked rows: straight into the device logits buffer
            class _A:
                __cuda_array_interface__ = dict(shape=(n, V), typestr="<f4", data=(int(lib.rwkv_logits_device(m._h)), False), version=2)
            view = torch.as_tensor(_A(), device="cuda:0")
        except Exception as e:                      # (no view: the host loop is left out, and said so)
            print(f"[constrain_bench] no view of the logits buffer: {e}", file=sys.stderr)

        def host(k):                                # the caller's loop the call replaces
            cur, q = list(first), [0] * n
            for step in range(k):
                rc = lib.rwkv_forward(m._h, (C.c_uint64 * n)(*cur), n, engine.MODE_PARRALEL)
                rc = rc or lib.rwkv_get_output(m._h, C.c_void_p(logits.ctypes.data), None, None, None, None, None, n)
                if rc:
                    raise RuntimeError(lib.rwkv_last_error().decode())
                lg = logits.reshape(n, V)
                c = np.full((n, V), -np.inf, np.float32)
                for s in range(n):
                    ids = tk[rp[q[s]]:rp[q[s] + 1]]
                    c[s, ids] = lg[s, ids]
                view.copy_(torch.from_numpy(c))
                torch.cuda.synchronize()
                for s in range(n):
                    cur[s] = m.sample_nucleus(u=((step * 7919 + s * 104729) % 1000) / 1000.0, row=s, slot=s, update=True, **NUC)
                    e = rp[q[s]] + int(np.searchsorted(tk[rp[q[s]]:rp[q[s] + 1]], cur[s]))
                    q[s] = int(nx[min(e, len(nx) - 1)])
            return cur

        if view is not None:
            host(2)
            hs = []
            for _ in range(max(2, args.reps // 2)):
                m.reset_state(); torch.cuda.synchronize()
                t0 = time.perf_counter()
                host(args.host_steps)
                hs.append(round((time.perf_counter() - t0) / args.host_steps * 1e3, 4))
            out["results"][f"{n}/host_nucleus"] = dict(host=hs)
            print(f"[constrain_bench:{args.child}] N={n} host loop: {np.median(hs):.3f} ms/step", file=sys.stderr, flush=True)
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
    line = dict(tool="constrain_bench", model=args.model, steps=args.steps, host_steps=args.host_steps, reps=args.reps, rounds=args.rounds,
                device=device, unit="ms per step", sparse=f"{SPARSE_STATES} states x {SPARSE_EDGES} edges", bias_entries=BIAS_N, results={})
    for case, ms in pooled.items():
        r = {name: stats(v) for name, v in ms.items()}
        if "until" in r:
            spread = lambda a, b: round(max(r[a]["max"] - r[a]["min"], r[b]["max"] - r[b]["min"]) * 1e3, 1)
            r["added_us_per_step"] = {name: dict(added=round((r[name]["median"] - r["until"]["median"]) * 1e3, 1), spread=spread(name, "until"))
                                      for name in ("everything", "sparse", "sparse_bias") if name in r}
            if "parent_until" in r:
                r["until_vs_parent_us_per_step"] = dict(added=round((r["until"]["median"] - r["parent_until"]["median"]) * 1e3, 1),
                                                        spread=spread("until", "parent_until"))
        line["results"][case] = r
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
