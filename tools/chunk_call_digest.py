#!/usr/bin/env python3
"""What every row layout of the chunk path leaves behind, as text that two builds of the engine can be compared on.

    RWKV_LIB=/path/to/lib_a.so python tools/chunk_call_digest.py > a.txt
    RWKV_LIB=/path/to/lib_b.so python tools/chunk_call_digest.py > b.txt         # diff a.txt b.txt must be empty
    python tools/chunk_call_digest.py --compare lib_a.so lib_b.so [--out DIR] [--timeout S]   # one process per library, then the comparison

The models, the start state and the named layouts are those of tests/segment_cases.py, at its four widths; the drafts are made with
tests/spec_cases.py.  Every case starts from the start state.  One line per case: the first 16 hex digits of SHA-256 of each of the five state
arrays over all slots, of the logits rows the call wrote, and of both together (segment_cases.digest).  The cases: rwkv_forward in GPT mode with
2, 33 and 65 rows and in PARRALEL mode with 40; rwkv_spec_verify with n_draft 0, 7 and 31, the draft being the greedy continuation with a wrong
id in the middle; rwkv_forward_segments with MIX32, MIX64, MIX77 and PAR40; MIX77 again in contexts made under RWKV_SEQ_ROWS=32 and under
RWKV_SEQ_STAGES=1."""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_cases():
    import numpy as np
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import segment_cases as sc
    import spec_cases as spc
    from rwkv_cpp_accelerated_amd import engine, modelfile as mf

    def dig(a):
        return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]

    for L, D in sc.WIDTHS:
        tensors = mf.synthetic_tensors(L, D, seed=sc.SEED + D)

        def context():
            m = engine.RWKV(resident=True)
            m.loadTensors(L, D, tensors, maxGPT=sc.MAXT)
            sc.start_state(engine, m, D)
            m.pull_state(sc.MAXT)
            return m, [a.copy() for a in m.state.arrays()]

        def restore(m, snap):
            for a, s in zip(m.state.arrays(), snap):
                a[:] = s
            m.push_state(sc.MAXT)

        def case(m, snap, name, call, n_rows):
            restore(m, snap)
            got = call()
            got = got if isinstance(got, tuple) else None       # spec_verify's (n_accepted, next)
            both = sc.digest(m, n_rows)[:16]            # (pulls the state)
            print(f"D={D} {name}:{'' if got is None else f' returned {got}'} state {' '.join(dig(a) for a in m.state.arrays())} "
                  f"logits {dig(m.logits(n_rows))} both {both}", flush=True)

        def ids(n):
            return [int(v) for v in np.random.default_rng(D + n).integers(1, sc.V, n)]

        m, snap = context()
        for n in (2, 33, 65):
            case(m, snap, f"rwkv_forward GPT {n} rows", lambda: m.forward(ids(n), engine.MODE_GPT), n)
        case(m, snap, "rwkv_forward PARRALEL 40 rows", lambda: m.forward(ids(40), engine.MODE_PARRALEL), 40)
        restore(m, snap)
        greedy = [int(t) for t in m.decode_greedy(101, spc.MAX_DRAFT)]        # what a verify behind token 101 confirms
        for n in (0, 7, 31):
            draft = greedy[:n]
            if n:
                draft[n // 2] = spc.wrong(draft[n // 2])
            case(m, snap, f"rwkv_spec_verify n_draft {n}", lambda: m.spec_verify(101, draft), n + 1)
        for name in ("MIX32", "MIX64", "MIX77", "PAR40"):
            case(m, snap, f"rwkv_forward_segments {name}", lambda: m.forward_segments(sc.tokens_for(sc.LAYOUTS[name], 77 + D)), sc.ROWS[name])
        m.close()
        for var, val in (("RWKV_SEQ_ROWS", "32"), ("RWKV_SEQ_STAGES", "1")):      # read when a context is made or first runs two passes
            os.environ[var] = val
            m, snap = context()
            case(m, snap, f"rwkv_forward_segments MIX77 under {var}={val}", lambda: m.forward_segments(sc.tokens_for(sc.LAYOUTS["MIX77"], 77 + D)),
                 sc.ROWS["MIX77"])
            m.close()
            del os.environ[var]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", nargs=2, metavar="LIB", help="run once per library (RWKV_LIB) in a process each and compare the two outputs as text")
    ap.add_argument("--out", default=None, help="with --compare: keep the two outputs as DIR/digest_a.txt and DIR/digest_b.txt")
    ap.add_argument("--timeout", type=float, default=240.0, help="with --compare: seconds each of the two processes may take")
    args = ap.parse_args()
    if not args.compare:
        return run_cases()
    texts = []
    for which, path in zip("ab", args.compare):
        try:        # a process that hangs is killed, and nothing more is started
            p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, RWKV_LIB=os.path.abspath(path)), stdout=subprocess.PIPE,
                               text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f"the process of {path} did not end within {args.timeout} s")
        if p.returncode != 0:
            sys.exit(f"the process of {path} failed with status {p.returncode}")       # nothing more is started
        texts.append(p.stdout)
        if args.out:
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, f"digest_{which}.txt"), "w") as f:
                f.write(p.stdout)
    a, b = (t.splitlines() for t in texts)
    differ = [i for i in range(max(len(a), len(b))) if i >= len(a) or i >= len(b) or a[i] != b[i]]
    print(texts[1], end="")
    print(f"== {len(a)} lines of {args.compare[0]} against {len(b)} of {args.compare[1]}: " + ("EQUAL as text" if not differ else f"{len(differ)} lines DIFFER"))
    for i in differ:
        print(f"  a: {a[i] if i < len(a) else '(none)'}\n  b: {b[i] if i < len(b) else '(none)'}")
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
