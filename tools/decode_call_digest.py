#!/usr/bin/env python3
"""What every generation call of the C ABI leaves behind, as text that two builds of the engine can be compared on.

    RWKV_LIB=/path/to/lib_a.so python tools/decode_call_digest.py > a.txt
    RWKV_LIB=/path/to/lib_b.so python tools/decode_call_digest.py > b.txt        # diff a.txt b.txt must be empty
    python tools/decode_call_digest.py --compare lib_a.so lib_b.so [--out DIR] [--timeout S]   # one process per library, then the comparison

The seeded synthetic model at the narrowest width that has a chunk path (L = 2, D = 64, max_ctx 8); every case starts from one fixed prompt
state (three PARRALEL steps of 8 streams), zero counts and the automaton states it names.  One line per case: the first 16 hex digits of
SHA-256 of ids / len / reason / steps_run, of the record arrays and the out states, of the five state arrays, the logits rows and the count
vectors.  The grid: N in {1, 3} x pick in {greedy, typical, typical recipe, nucleus with penalties} x hooks in {none, stop + budget that fires, record with
top_n 3, constraint with a bias, all three}, the all-three case also as a KEEP continuation, and the three one-stream entry points.  Then a
block of refused calls, each with its status and rwkv_last_error() text; most of them carry two faults at once, so the order of an entry
point's checks shows."""
import argparse
import ctypes as C
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, D, CTX, STEPS, TOPN = 2, 64, 8, 12, 3
PICKS = {"greedy": dict(pick="greedy"), "typical": dict(pick="typical", temp=0.9, tau=0.8),
         "typical recipe": dict(pick="typical", temp=0.9, tau=0.8, recipe=True),      # default mode has no select: this one runs it
         "nucleus": dict(pick="nucleus", temp=1.0, top_p=0.9, presence=0.4, frequency=0.4, decay=0.996)}
EDGES = 48


def dig(*arrays):
    import numpy as np
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def automata(np, V):
    """(ending, loop): four states of EDGES edges each; in `ending` a fifth, terminal state is the target of about one edge in five"""
    rng = np.random.default_rng(11)
    tok = np.concatenate([np.sort(rng.choice(np.arange(1, V), EDGES, replace=False)) for _ in range(4)]).astype(np.uint32)
    ending = (np.array([0, EDGES, 2 * EDGES, 3 * EDGES, 4 * EDGES, 4 * EDGES], np.uint32), tok, rng.integers(0, 5, tok.size).astype(np.uint32))
    loop = (np.arange(0, tok.size + 1, EDGES, dtype=np.uint32), tok, rng.integers(0, 4, tok.size).astype(np.uint32))
    return ending, loop


def run_cases():
    import numpy as np
    sys.path.insert(0, ROOT)
    from rwkv_cpp_accelerated_amd import engine, modelfile as mf
    V = mf.VOCAB
    lib = engine.lib()
    m = engine.RWKV(resident=True)
    m.loadTensors(L, D, mf.synthetic_tensors(L, D, seed=41, head_scale=30.0), maxGPT=CTX)
    rng = np.random.default_rng(5)
    for _ in range(3):
        m.forward([int(v) for v in rng.integers(1, V, CTX)], engine.MODE_PARRALEL)
    m.pull_state(CTX)
    snap = [a.copy() for a in m.state.arrays()]
    ending, loop = automata(np, V)

    def restore():
        for a, s in zip(m.state.arrays(), snap):
            a[:] = s
        m.push_state(CTX)
        for s in range(CTX):
            m.penalty_set(s, None)

    def left(n):
        m.pull_state(CTX)
        st = [a.copy() for a in m.state.arrays()]
        return (f"state {' '.join(dig(a) for a in st)} logits {dig(m.logits(n))} counts {dig(*[m.penalty_get(s) for s in range(n)])} "
                f"q {dig(m.constraint_state_get(0, n))}")

    def line(name, r):
        """r: the tuple a decode_batch_* wrapper returns (ids, len, reason, steps_run, [out states], [logprob, entropy, top_ids, top_logprob])"""
        n = r[0].shape[0]
        head = f"ids {dig(r[0])}"
        if len(r) > 1:
            head += f" len {dig(r[1])} reason {dig(r[2])} steps_run {r[3]}"
        rest = list(r[4:])
        if rest and rest[0].ndim == 1:
            head += f" out_state {dig(rest.pop(0))}"
        if rest:
            head += f" record {' '.join(dig(a) for a in rest)}"
        print(f"{name}: {head} {left(n)}", flush=True)

    def stop_of(r, budgets=(7, 2, 9)):
        """a two-id stop sequence out of stream 0's own ids that completes at step 5 at the latest, and budgets of which one fires"""
        n, ln = r[0].shape[0], int(min(r[1][0], 5))
        return dict(stops=[[int(v) for v in r[0][0][max(0, ln - 2):ln]]], max_new=list(budgets[:n]))

    for n in (1, 3):
        first = [int(v) for v in np.random.default_rng(3).integers(1, V, n)]
        seeds = [1000 + 7 * s for s in range(n)]
        q0 = [s % 4 for s in range(n)]
        bias = [{int(ending[1][ending[0][q0[s]]]): -np.inf, int(ending[1][ending[0][q0[s]] + 1]): 2.0, 7 + s: 3.0} for s in range(n)]
        for pick, kw in PICKS.items():
            tag = f"N={n} {pick}"
            kw = dict(kw, seeds=seeds)
            m.constraint_clear()
            restore()
            plain = {"greedy": m.decode_batch_greedy, "typical": m.decode_batch_typical, "nucleus": m.decode_batch_nucleus}[kw["pick"]]
            line(f"{tag} none", (plain(first, STEPS, **({} if pick == "greedy" else {k: v for k, v in kw.items() if k != "pick"})),))
            restore()
            full = m.decode_batch_until(first, STEPS, **kw)
            line(f"{tag} until without a stop", full)
            restore()
            line(f"{tag} stop", m.decode_batch_until(first, STEPS, **stop_of(full), **kw))
            restore()
            line(f"{tag} record", m.decode_batch_logprobs(first, STEPS, top_n=TOPN, **kw))
            restore()
            line(f"{tag} stop + record", m.decode_batch_logprobs(first, STEPS, top_n=TOPN, **stop_of(full), **kw))
            if kw["pick"] == "typical":
                continue                            # typical under a constraint is a refusal: in the block below
            restore()
            line(f"{tag} constraint (implicit state) + bias", m.decode_batch_constrained(first, STEPS, bias=bias, **kw))
            m.constraint_set(*ending)
            restore()
            con = m.decode_batch_constrained(first, STEPS, start=q0, bias=bias, **kw)
            line(f"{tag} constraint + bias", con)
            restore()
            line(f"{tag} all three", m.decode_batch_constrained(first, STEPS, start=q0, bias=bias, logprobs=True, top_n=TOPN, **stop_of(con), **kw))
            m.constraint_set(*loop)
            restore()
            con = m.decode_batch_constrained(first, STEPS, start=q0, bias=bias, **kw)
            restore()
            a = m.decode_batch_constrained(first, STEPS // 2, start=q0, bias=bias, logprobs=True, top_n=TOPN, **stop_of(con, (6, 2, 5)), **kw)
            line(f"{tag} all three, first half", a)
            fed = [int(a[0][s][a[1][s] - 1]) for s in range(n)]
            kw2 = dict(kw, seeds=[s + STEPS // 2 for s in seeds])
            line(f"{tag} all three, KEEP continuation", m.decode_batch_constrained(fed, STEPS // 2, start=None, bias=bias, logprobs=True, top_n=TOPN,
                                                                                  keep=True, **stop_of(con, (6, 2, 5)), **kw2))
    m.constraint_clear()
    restore()
    line("one stream, rwkv_decode_greedy", (m.decode_greedy(11, STEPS).reshape(1, -1),))
    restore()
    line("one stream, rwkv_decode_typical", (m.decode_typical(11, STEPS, temp=0.9, tau=0.8, seed=7).reshape(1, -1),))
    restore()
    line("one stream, rwkv_decode_nucleus", (m.decode_nucleus(11, STEPS, seed=7, **{k: v for k, v in PICKS["nucleus"].items() if k != "pick"}).reshape(1, -1),))
    restore()
    x = m.decode_nucleus(11, STEPS // 2, seed=7, **{k: v for k, v in PICKS["nucleus"].items() if k != "pick"})
    y = m.decode_nucleus(int(x[-1]), STEPS // 2, seed=13, keep=True, **{k: v for k, v in PICKS["nucleus"].items() if k != "pick"})
    line("one stream, rwkv_decode_nucleus, KEEP continuation", (np.concatenate([x, y]).reshape(1, -1),))

    # ---- refused calls: status and text; nothing is launched ----
    print("== refused calls ==", flush=True)
    u64, u32, dbl = C.c_uint64, C.c_uint32, C.c_double
    h = m._h
    BAD = V                                         # a token id out of range
    m.constraint_set(*ending)
    restore()

    def refused(name, rc):
        print(f"{name}: status {int(rc)} \"{lib.rwkv_last_error().decode(errors='replace')}\"", flush=True)

    def pk(kind, temp=1.0, flags=0, reserved=0):
        p = engine.Pick(kind, float(temp), 0.8, 0, engine.nucleus_params(temp, 0.9, 0, 0.4, 0.4, 0.996, flags))
        p.nucleus.reserved = reserved
        return p

    def sp(flags=0, reserved=0, max_new=None, seqs=()):
        s, alive = engine.stop_params(seqs, max_new)
        s.flags, s.reserved = flags, reserved
        return s, alive

    def lpo(top_n=0, reserved=0, ids=None, lp=True):
        """ids: whether top_ids and top_logprob are there (None: as top_n asks)"""
        e = 3 * 4 * max(1, top_n)
        alive = ((dbl * e)(), (dbl * e)(), (u64 * e)(), (dbl * e)())
        ids = top_n > 0 if ids is None else ids
        return engine.LogprobOut(top_n, reserved, alive[0] if lp else None, alive[1], alive[2] if ids else None, alive[3] if ids else None), alive

    def until(name, first, n, steps, pick, stop, ln=True):
        out, l, r, ran = (u64 * 64)(), (u32 * 8)(), (u32 * 8)(), u64(0)
        refused(f"rwkv_decode_batch_until: {name}", lib.rwkv_decode_batch_until(h, (u64 * 8)(*first), n, steps, C.byref(pick), (u64 * 8)(), C.byref(stop[0]), out,
                                                                                l if ln else None, r, C.byref(ran)))

    def logprobs(name, first, n, steps, pick, stop, rec, ln=True):
        out, l, r, ran = (u64 * 64)(), (u32 * 8)(), (u32 * 8)(), u64(0)
        refused(f"rwkv_decode_batch_logprobs: {name}", lib.rwkv_decode_batch_logprobs(h, (u64 * 8)(*first), n, steps, C.byref(pick), (u64 * 8)(),
                                                                                      None if stop is None else C.byref(stop[0]), C.byref(rec[0]), out,
                                                                                      l if ln else None, r, C.byref(ran)))

    def constrained(name, first, n, steps, pick, cp, stop=None, rec=None):
        out, l, r, ran = (u64 * 64)(), (u32 * 8)(), (u32 * 8)(), u64(0)
        refused(f"rwkv_decode_batch_constrained: {name}", lib.rwkv_decode_batch_constrained(h, (u64 * 8)(*first), n, steps, C.byref(pick), (u64 * 8)(), C.byref(cp),
                                                                                            None if stop is None else C.byref(stop[0]),
                                                                                            None if rec is None else C.byref(rec[0]), out, l, r, C.byref(ran)))

    def cparams(start=None, reserved=0, bias=None):
        st = None if start is None else (u32 * 8)(*start)
        bp = bt = bv = None
        if bias is not None:
            bp, bt, bv = (u32 * 8)(*bias[0]), (u32 * 8)(*bias[1]), (C.c_float * 8)(*bias[2])
        return engine.ConstrainParams(st, bp, bt, bv, None, reserved)

    G, T, N_ = engine.PICK_GREEDY, engine.PICK_TYPICAL, engine.PICK_NUCLEUS
    until("unknown pick kind 7, n_steps 0", [5, 6], 2, 0, pk(7), sp())
    until("n_streams 0, unknown stop flag bits", [5], 0, 4, pk(G), sp(flags=6))
    until("n_streams 9 of 8, n_steps 0", [5], 9, 0, pk(G), sp())
    until("n_steps 0, token id out of range", [5, BAD], 2, 0, pk(G), sp())
    until("n_steps 70000, typical temp 0", [5], 1, 70000, pk(T, temp=0.0), sp())
    until("token id out of range, nucleus reserved 1", [BAD], 1, 4, pk(N_, reserved=1), sp())
    until("typical temp 0, stop reserved 1", [5], 1, 4, pk(T, temp=0.0), sp(reserved=1))
    until("stop reserved 1, budget 9 of 4 steps", [5, 6], 2, 4, pk(G), sp(reserved=1, max_new=[9, 1]))
    until("stop sequence of length 0, budget 0", [5, 6], 2, 4, pk(G), sp(max_new=[0, 1], seqs=[[3, 4], []]))
    until("stop id out of range, budget 0", [5, 6], 2, 4, pk(G), sp(max_new=[0, 1], seqs=[[3, BAD]]))
    until("out_len NULL, unknown pick kind -1", [5], 1, 4, pk(-1), sp(), ln=False)
    logprobs("top_n 33, reserved 1", [5], 1, 4, pk(G), sp(), lpo(33, 1))
    logprobs("top_n 2 without top_ids, reserved 1", [5], 1, 4, pk(G), sp(), lpo(2, 1, ids=False))
    logprobs("reserved 1, unknown pick kind 3", [5], 1, 4, pk(3), sp(), lpo(0, 1))
    logprobs("unknown pick kind 3, n_steps 0", [5], 1, 0, pk(3), None, lpo(2))
    logprobs("n_steps 0, stop reserved 1", [5], 1, 0, pk(G), sp(reserved=1), lpo(2))
    logprobs("a stop without out_len, top_n 33", [5], 1, 4, pk(G), sp(), lpo(33), ln=False)
    logprobs("logprob NULL, top_n 33", [5], 1, 4, pk(G), None, lpo(33, lp=False))
    logprobs("n_streams 0, top_n 33", [5], 0, 4, pk(G), None, lpo(33))
    constrained("top_n 33, constraint reserved 1", [5], 1, 4, pk(G), cparams(reserved=1), rec=lpo(33))
    constrained("top_n 0 with top_ids, record reserved 1", [5], 1, 4, pk(G), cparams(), rec=lpo(0, 1, ids=True))
    constrained("record reserved 1, unknown pick kind 9", [5], 1, 4, pk(9), cparams(), rec=lpo(0, 1))
    constrained("unknown pick kind 9, n_steps 0", [5], 1, 0, pk(9), cparams())
    constrained("typical, constraint reserved 1", [5], 1, 4, pk(T), cparams(reserved=1))
    constrained("typical temp 0, constraint reserved 1", [5], 1, 4, pk(T, temp=0.0), cparams(reserved=1))
    constrained("typical, start state 9 of 5", [5], 1, 4, pk(T), cparams(start=[9]))
    constrained("typical N=3, a stop and a record", [5, 6, 7], 3, 4, pk(T), cparams(start=[0, 1, 2]), stop=sp(max_new=[1, 2, 3]), rec=lpo(3))
    constrained("stop reserved 1, start state 9 of 5", [5], 1, 4, pk(G), cparams(start=[9]), stop=sp(reserved=1))
    constrained("bias_ptr without bias_tok, terminal start state 4", [5], 1, 4, pk(G), engine.ConstrainParams((u32 * 8)(4), (u32 * 8)(), None, None, None, 0))
    constrained("bias ids descending, terminal start state 4", [5, 6], 2, 4, pk(G), cparams(start=[0, 4], bias=([0, 2, 2], [9, 8], [1.0, 1.0])))
    constrained("bias_ptr[0] = 1, start state 9 of 5", [5], 1, 4, pk(G), cparams(start=[9], bias=([1, 2], [9, 8], [1.0, 1.0])))
    constrained("start state 9 of 5, nucleus temp 0", [5], 1, 4, pk(N_, temp=0.0), cparams(start=[9]))
    constrained("a record of more than 2^22 entries, start state 9 of 5", [5] * 8, 8, 65536, pk(G), cparams(start=[9] * 8), rec=lpo(32))

    def pickc(name, row, slot, pick, u=0.5, bias=None):
        tok, q = u64(0), u32(0)
        refused(f"rwkv_pick_constrained: {name}", lib.rwkv_pick_constrained(h, row, slot, C.byref(pick), None if bias is None else C.byref(bias), u, 1,
                                                                            C.byref(tok), C.byref(q)))

    bt, bv = (u32 * 4)(9, 8), (C.c_float * 4)(1.0, 1.0)
    pickc("row 8 of 8, typical", 8, 0, pk(T))
    pickc("slot 9 of 8, unknown pick kind 5", 0, 9, pk(5))
    pickc("typical, u = 2", 0, 0, pk(T), u=2.0)
    pickc("nucleus temp 0, u = 2", 0, 0, pk(N_, temp=0.0), u=2.0)
    pickc("nucleus u = 2, bias reserved 1", 0, 0, pk(N_), u=2.0, bias=engine.Bias(2, 1, bt, bv))
    pickc("bias reserved 1, bias ids descending", 0, 0, pk(G), bias=engine.Bias(2, 1, bt, bv))
    m.constraint_state_set([4], 3)
    pickc("bias ids descending, the slot on a terminal state", 0, 3, pk(G), bias=engine.Bias(2, 0, bt, bv))
    pickc("greedy u = 2 (not read), the slot on a terminal state", 0, 3, pk(G), u=2.0)
    m.constraint_state_set([0], 3)

    def nucleus_args(temp=1.0, top_p=0.9, decay=0.996, flags=0, reserved=0):
        p = engine.nucleus_params(temp, top_p, 0, 0.4, 0.4, decay, flags)
        p.reserved = reserved
        return p

    tok, out = u64(0), (u64 * 64)()
    refused("rwkv_sample_nucleus: row 8 of 8, temp 0", lib.rwkv_sample_nucleus(h, 8, 0, C.byref(nucleus_args(temp=0.0)), 0.5, C.byref(tok)))
    refused("rwkv_sample_nucleus: slot 8 of 8, u = 2", lib.rwkv_sample_nucleus(h, 0, 8, C.byref(nucleus_args()), 2.0, C.byref(tok)))
    refused("rwkv_sample_nucleus: temp 0, u = 2", lib.rwkv_sample_nucleus(h, 0, 0, C.byref(nucleus_args(temp=0.0)), 2.0, C.byref(tok)))
    refused("rwkv_sample_nucleus: decay 2, unknown flag bits", lib.rwkv_sample_nucleus(h, 0, 0, C.byref(nucleus_args(decay=2.0, flags=8)), 0.5, C.byref(tok)))
    refused("rwkv_sample_nucleus: reserved 1, u = -1", lib.rwkv_sample_nucleus(h, 0, 0, C.byref(nucleus_args(reserved=1)), -1.0, C.byref(tok)))
    refused("rwkv_decode_nucleus: token id out of range, n_tokens 0", lib.rwkv_decode_nucleus(h, BAD, 0, C.byref(nucleus_args()), 7, out))
    refused("rwkv_decode_nucleus: n_tokens 0, temp 0", lib.rwkv_decode_nucleus(h, 5, 0, C.byref(nucleus_args(temp=0.0)), 7, out))
    refused("rwkv_decode_nucleus: n_tokens 65537, top_p nan", lib.rwkv_decode_nucleus(h, 5, 65537, C.byref(nucleus_args(top_p=float("nan"))), 7, out))
    refused("rwkv_decode_nucleus: params NULL, n_tokens 0", lib.rwkv_decode_nucleus(h, 5, 0, None, 7, out))
    refused("rwkv_decode_greedy: token id out of range, n_tokens 0", lib.rwkv_decode_greedy(h, BAD, 0, out))
    refused("rwkv_decode_greedy: n_tokens 65537", lib.rwkv_decode_greedy(h, 5, 65537, out))
    refused("rwkv_decode_typical: n_tokens 0, temp 0", lib.rwkv_decode_typical(h, 5, 0, 0.0, 0.8, 7, 0, out))
    refused("rwkv_decode_typical: token id out of range, temp 0", lib.rwkv_decode_typical(h, BAD, 4, 0.0, 0.8, 7, 0, out))
    refused("rwkv_decode_batch_greedy: n_streams 0, n_steps 0", lib.rwkv_decode_batch_greedy(h, (u64 * 8)(5), 0, 0, out))
    refused("rwkv_decode_batch_typical: n_steps 0, temp 0", lib.rwkv_decode_batch_typical(h, (u64 * 8)(5), 1, 0, 0.0, 0.8, (u64 * 8)(), 0, out))
    refused("rwkv_decode_batch_typical: seeds NULL, n_steps 0", lib.rwkv_decode_batch_typical(h, (u64 * 8)(5), 1, 0, 0.9, 0.8, None, 0, out))
    refused("rwkv_decode_batch_nucleus: params NULL, n_streams 0", lib.rwkv_decode_batch_nucleus(h, (u64 * 8)(5), 0, 4, None, (u64 * 8)(), out))
    refused("rwkv_decode_batch_nucleus: token id out of range, decay 2", lib.rwkv_decode_batch_nucleus(h, (u64 * 8)(5, BAD), 2, 4, C.byref(nucleus_args(decay=2.0)),
                                                                                                      (u64 * 8)(), out))

    def scan(name, n, steps, first, stop, planted=5):
        l, r = (u32 * 8)(), (u32 * 8)()
        refused(f"rwkv_debug_stop_scan: {name}", lib.rwkv_debug_stop_scan(h, (u64 * 64)(*([planted] * 64)), (u64 * 8)(*first), n, steps, C.byref(stop[0]), l, r))

    scan("n 0, steps 0", 0, 0, [5], sp())
    scan("steps 0, token id out of range", 2, 0, [5, BAD], sp())
    scan("steps 65537, stop reserved 1", 1, 65537, [5], sp(reserved=1))
    scan("token id out of range, planted id out of range", 1, 4, [BAD], sp(), planted=BAD)
    scan("planted id out of range, stop reserved 1", 1, 4, [5], sp(reserved=1), planted=BAD)

    def beam(name, first, steps, width, n_stop=0, stops=(5,), reserved=0):
        bp, alive = engine.beam_params(width, stops)
        bp.n_stop, bp.reserved = n_stop, reserved
        tokens, ln, score = (u64 * 1024)(), (u32 * 16)(), (dbl * 16)()
        refused(f"rwkv_decode_beam: {name}", lib.rwkv_decode_beam(h, first, steps, C.byref(bp), C.byref(engine.BeamOut(tokens, ln, score, None))))

    beam("width 1, n_steps 0", 5, 0, 1)
    beam("width 9 of 8, n_steps 0", 5, 0, 9)
    beam("17 stop ids, n_steps 0", 5, 0, 2, n_stop=17)
    beam("reserved 1, n_steps 0", 5, 0, 2, reserved=1)
    beam("stop id 0, n_steps 0", 5, 0, 2, n_stop=1, stops=(0,))
    beam("n_steps 0, token id out of range", BAD, 0, 2)
    beam("n_steps 65537, token id out of range", BAD, 65537, 2)
    beam("token id out of range", BAD, 4, 2)

    st = (u32 * 8)(9, 9)
    refused("rwkv_constraint_state_set: n 0, state 9 of 5", lib.rwkv_constraint_state_set(h, 0, 0, st))
    refused("rwkv_constraint_state_set: slot 8 of 8, state 9 of 5", lib.rwkv_constraint_state_set(h, 8, 1, st))
    refused("rwkv_constraint_state_set: slots 7 .. + 2, state 9 of 5", lib.rwkv_constraint_state_set(h, 7, 2, st))
    refused("rwkv_constraint_state_set: state 9 of 5", lib.rwkv_constraint_state_set(h, 0, 2, st))
    refused("rwkv_constraint_state_get: n 0", lib.rwkv_constraint_state_get(h, 0, 0, st))
    refused("rwkv_constraint_state_get: slots 7 .. + 2", lib.rwkv_constraint_state_get(h, 7, 2, st))
    refused("rwkv_constraint_state_get: slot0 2^64 - 1, n 2", lib.rwkv_constraint_state_get(h, 2 ** 64 - 1, 2, st))
    print(f"after the refused calls: {left(CTX)}", flush=True)
    m.constraint_clear()
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", nargs=2, metavar="LIB", help="run once per library (RWKV_LIB) in a process each and compare the two outputs as text")
    ap.add_argument("--out", default=None, help="with --compare: keep the two outputs as DIR/digest_a.txt and DIR/digest_b.txt")
    ap.add_argument("--timeout", type=float, default=120.0, help="with --compare: seconds each of the two processes may take")
    args = ap.parse_args()
    if not args.compare:
        return run_cases()
    texts = []
    for which, path in zip("ab", args.compare):
        try:        # a process runs for some ten seconds; one that hangs is killed, and nothing more is started
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
