#!/usr/bin/env python3
"""Speculative greedy decoding at 7B shapes: what a verify costs against rwkv_forward of the same rows on the parent commit, and what a round of
the loop costs with a draft that is always right, one that is always wrong, and the host-side lookup drafter.

    python tools/spec_bench.py --parent-lib <librwkv_mi355x.so of the parent commit> [--model 7B] [--draft 169M] [--n-drafts 0,1,3,7,15,31]
                               [--reps 5] [--iters 8] [--tokens 96] [--ks 4,8] [--out profiles/spec]

Three 7B contexts in one process with the same synthetic weights: THIS tree's library twice -- the target and the always-right draft -- and the
parent commit's (--parent-lib, a second dlopen bound here to the entry points the legs need), so that the legs alternate inside one run.
  verify   per n_draft: (A) parent rwkv_forward of the n_draft + 1 rows in GPT mode (n_draft = 0: ONE row, which the parent runs on its decode
           kernels -- the chunk path had no one-row entry), (B) rwkv_spec_verify with a draft that is wrong at once (a = 0; the commit moves the
           same bytes whatever a is).  (B) - (A) is what checkpoints, picks, accept and commit cost.  --reps rounds of A, B in turn after a
           warm round; a round is --iters calls; ms per call, median and min .. max.  (Whether the verify pass should be a captured graph was
           measured with an earlier form of this tool on a build that could do both: profiles/spec/graph_vs_direct.txt.)
  step     the decode step of this tree in the same process (rwkv_decode_greedy, 64 ids), for the break-even: a round of k drafts pays when it
           emits more than verify(k) / step ids, the draft's own cost not counted.
  loop     rwkv_decode_speculative of --tokens ids per k of --ks with (a) the second 7B context as the draft (acceptance 1: the best case's
           round), (b) a --draft shaped model of another seed (acceptance ~ 0: the worst case), and RWKV.decode_lookup; ms per round, ids per
           round, ms per id, and the round's parts timed on their own: the draft's k + 1 steps with their k + 1 slot copies, the verify, the
           restore of the draft's slot 0.
Wall clock around synchronous calls: every leg ends in a stream synchronise.  Synthetic weights: acceptance on real text is NOT measured here."""
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
    """the parent commit's library: rwkv_forward, bound by hand (this tree's binding asks for symbols it does not have)"""

    def __init__(self, path, L, D, tensors, max_ctx):
        vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
        lib = self.lib = C.CDLL(path)
        assert not hasattr(lib, "rwkv_spec_verify"), "--parent-lib is not the parent's library: it has rwkv_spec_verify"
        lib.rwkv_create.argtypes = [C.POINTER(vp), i32]
        lib.rwkv_load_tensors.argtypes = [vp, u64, u64, C.POINTER(vp), i32, u64]
        lib.rwkv_reset_state.argtypes = [vp]
        lib.rwkv_forward.argtypes = [vp, C.POINTER(u64), u64, i32]
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

    def forward(self, rows):
        self.chk(self.lib.rwkv_forward(self.h, (C.c_uint64 * len(rows))(*rows), len(rows), engine.MODE_GPT))

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
    ap.add_argument("--draft", default="169M")
    ap.add_argument("--n-drafts", default="0,1,3,7,15,31")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--tokens", type=int, default=96)
    ap.add_argument("--ks", default="4,8")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n_drafts = [int(x) for x in args.n_drafts.split(",")]
    ks = [int(x) for x in args.ks.split(",")]
    L, D = mf.SHAPES[args.model]
    max_ctx = 34
    engine.lib()
    t = mf.synthetic_tensors_torch(L, D, seed=0)
    m, same = engine.RWKV(resident=True), engine.RWKV(resident=True)
    m.loadTensors(L, D, t, maxGPT=max_ctx)
    same.loadTensors(L, D, t, maxGPT=max_ctx)
    parent = Parent(os.path.abspath(args.parent_lib), L, D, t, max_ctx)
    del t
    torch.cuda.empty_cache()
    Ld, Dd = mf.SHAPES[args.draft]
    small = engine.RWKV(resident=True)
    small.loadTensors(Ld, Dd, mf.synthetic_tensors_torch(Ld, Dd, seed=1), maxGPT=max_ctx)
    line = dict(tool="spec_bench", model=args.model, n_layers=L, n_embed=D, draft=args.draft, reps=args.reps, iters=args.iters, tokens=args.tokens,
                maxGPT=max_ctx, device=torch.cuda.get_device_name(0), verify={}, loop={})
    text = []

    def say(msg):
        text.append(msg)
        print("[spec_bench] " + msg, file=sys.stderr, flush=True)

    # ---- the decode step of this tree, same process ----
    m.reset_state()
    m.decode_greedy(5, 64)
    step = stats([timed(lambda: m.decode_greedy(5, 64), 64) for _ in range(args.reps)])
    line["decode_step_ms"] = step
    say(f"decode step (rwkv_decode_greedy, 64 ids): {fmt(step)}")

    # ---- verify cost ----
    rng = np.random.default_rng(3)
    for nd in n_drafts:
        rows = [int(v) for v in rng.integers(2, mf.VOCAB, nd + 1)]
        legs = dict(parent_forward=lambda: parent.forward(rows), verify=lambda: m.spec_verify(rows[0], rows[1:]))
        for fn in legs.values():
            fn()
        got = {k: [] for k in legs}
        for _ in range(args.reps):
            for k, fn in legs.items():
                got[k].append(timed(lambda: [fn() for _ in range(args.iters)], args.iters))
        r = {k: stats(v) for k, v in got.items()}
        r["added_ms"] = round(r["verify"]["median"] - r["parent_forward"]["median"], 4)
        r["spread_ms"] = round(max(max(v) - min(v) for v in got.values()), 4)
        r["break_even_ids_per_round"] = round(r["verify"]["median"] / step["median"], 2)
        line["verify"][str(nd)] = r
        say(f"n_draft={nd}: parent forward of {nd + 1} rows {fmt(r['parent_forward'])}, verify {fmt(r['verify'])} (added {r['added_ms']:+.3f} ms), "
            f"spread {r['spread_ms']:.3f} ms, "
            f"break-even {r['break_even_ids_per_round']:.2f} ids per round")

    # ---- loop cost ----
    prompt = [int(v) for v in np.random.default_rng(5).integers(2, mf.VOCAB, 8)]

    def prefill(*models):
        for x in models:
            x.reset_state()
            x.forward(prompt, engine.MODE_GPT)

    lib = engine.lib()
    for k in ks:
        res = {}
        for name, dm in (("same_weights", same), ("small_other_seed", small), ("lookup", None)):
            def run():
                prefill(m, *([dm] if dm is not None else []))
                t0 = time.perf_counter()
                ids, st = m.decode_lookup(prompt + [5], args.tokens, k=k, n=2) if dm is None else m.decode_speculative(dm, 5, args.tokens, k)
                return (time.perf_counter() - t0) * 1e3, st
            run()
            runs = [run() for _ in range(args.reps)]
            st = runs[0][1]
            res[name] = dict(ms_per_round=stats([ms / st["rounds"] for ms, _ in runs]), ms_per_id=stats([ms / args.tokens for ms, _ in runs]),
                             rounds=st["rounds"], drafted=st["drafted"], accepted=st["accepted"], ids_per_round=round(args.tokens / st["rounds"], 3),
                             acceptance=round(st["accepted"] / max(1, st["drafted"]), 4))
            # the round's parts on their own (full-length rounds: k drafts)
            if dm is not None:
                prefill(m, dm)
                copy = lambda d, s: engine._chk(lib.rwkv_state_copy(dm._h, d, s))
                res[name]["draft_ms"] = stats([timed(lambda: (dm.decode_greedy(5, k + 1), [copy(i + 1, 0) for i in range(k + 1)])) for _ in range(args.reps + 1)][1:])
                res[name]["rollback_ms"] = stats([timed(lambda: copy(0, 1)) for _ in range(args.reps + 1)][1:])
            d = [int(v) for v in rng.integers(2, mf.VOCAB, k)]
            res[name]["verify_ms"] = stats([timed(lambda: m.spec_verify(5, d)) for _ in range(args.reps + 1)][1:])
            r = res[name]
            parts = (f"draft {fmt(r['draft_ms'])}, verify {fmt(r['verify_ms'])}, rollback {fmt(r['rollback_ms'])}" if dm is not None
                     else f"verify {fmt(r['verify_ms'])} (the drafter runs on the host)")
            say(f"k={k} {name}: {r['rounds']} rounds for {args.tokens} ids, acceptance {r['acceptance']:.3f}, {r['ids_per_round']:.2f} ids per round, "
                f"round {fmt(r['ms_per_round'])}, per id {fmt(r['ms_per_id'])} against the decode step's {step['median']:.3f} ms; parts: {parts}")
        line["loop"][str(k)] = res
    line["resident_bytes"] = m.resident_bytes()
    parent.close()
    for x in (m, same, small):
        x.close()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "spec_bench.json"), "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")
        with open(os.path.join(args.out, "spec_bench.txt"), "w") as f:
            f.write("\n".join(text) + "\n")
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
