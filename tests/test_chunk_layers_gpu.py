"""Layer-by-layer parity of the CHUNK path (csrc/seq.hip.h) at the decode kernels' tolerance: what tests/test_kernels_gpu.py is to the
decode kernels.  A context restricted to ONE layer (rwkv_set_layer_range) runs a chunk through rwkv_stage_chunk on residual rows
written into rwkv_xseq_device and on recurrent state pushed into slot 0 -- inputs no token sequence reaches -- and every row of its
output and the state it leaves are compared with oracle_stage_forward (oracle/rwkv_oracle.c), called row after row on a copy of the same
rows and state.  The PARRALEL step, which reaches these kernels only through a whole-model context, is held to the same bounds through
the state of both layers of an L = 2 model.

Legs and bounds (parity.TOL = 3e-5 of the vector's max |.|, the number and the reason of the decode suite):
   update   per row, x_out - x_in within TOL max |update| + 2^-23 max |x_in|: the reference rounds f32(x) + att_out . y to f32
            (rwkv.cu:548), two correct implementations may differ by that ulp of the accumulator when |x| is large
   xy       TOL: ln1 of the chunk's last row, an input the test planted
   aa, bb   1e-4, as in tests/test_kernels_gpu.py (f64 recurrences behind exp of an f32 k); case f, where the vector's max hides all
            but the top decade, adds both ELEMENT BY ELEMENT at 1e-4: bb relative to itself (bb' = (bb + e^k) e^w is a sum of positive
            terms: every element is as well conditioned as the largest), aa relative to the sum of the magnitudes of its terms plus
            TOL of the rows' max |v| under the same weights (chunk_cases.aa_elem_err has the derivation)
   pp       bit-equal to what was pushed (rwkv.cu:257)
   dd       = ln2(x_mid), one LayerNorm behind the vector between att_out and the channel mix, which cannot be read back.  x_mid is
            allowed eps = TOL max |x_mid - x_in| + 2^-23 max |x_in| like any residual vector behind an update; through the LayerNorm
            that is |w_i| (eps / sd) (2 + sqrt(D / (D - 1)) |z_i|) per element (derivation: chunk_cases.ln_leg_bound, checked
            numerically in tests/test_chunk_cases_cpu.py), with sd, z of the ORACLE's x_mid (its att_out half, chunk_cases.oracle_att_half).
            Bound = TOL + max_i of that / max |dd|: 4e-5 .. 6e-5 on the baseline, more only where |x_in|, the update or 1 / sd is large
            (every test prints it as `dd cap`).
   logits   last stage: rows [row0, row0 + n) against oracle.layernorm + oracle.mm8_layer(HEAD) of the ENGINE's own output rows, TOL
            (k_seq_gemm_ks isolated from everything before it)
   PARRALEL layer 1's xy = ln1(layer 0's output) and both dd's are bounded like dd, from the allowances of the updates in front of them
            (test_parralel_step_...); logits by parity.check_logits; slots >= N bit-equal.
tests/test_chunk_cases_cpu.py holds the oracle itself to HALF of each bound against a plain f64 evaluation of the same inputs, so a
failure here is the engine's.

Which test reaches which kernel of seq.hip.h (every kernel a forward call can launch):
   k_seq_embed                               test_first_stage_...  (ids 0, VOCAB - 1, a repeated id), test_parralel_step_...
   k_seq_resid<0> / <1> / <2>                every test (statistics of the incoming rows / behind att_out / behind ffn_v)
   k_seq_site<3> / <2>                       every test;  k_seq_site<1> (ln_out): test_last_stage_..., test_parralel_step_...
   k_seq_wkv<32>                             chunks of n <= 32;  k_seq_wkv<64>: chunks of n > 32; its PARRALEL branch: test_parralel_step_...
   k_seq_stage<0> / <1>                      every test
   k_seq_gemm_p<0|1|2, .., 8, ..>            n <= 32 at D <= 4096;  the 10-k-block instances: n <= 32 at D = 4160, 5056, 5120
   k_seq_gemm_p<3, 1, 4, 1, 4, true>         every chunk of n <= 32 (ffn_v)
   k_seq_gemm_p<.., 2> (two halves)          n > 32: att_out and ffn_v at every width, K/V/R below 4096, ffn k/r below 1536
   k_seq_gemm_b<2, ..>                       n > 32 at D >= 1536 (ffn k/r);  k_seq_gemm_b<0, ..>: n > 32 at D >= 4096 (K/V/R)
   k_seq_gemm_ks                             test_last_stage_... (once per half; row0 > 0 once), test_parralel_step_...
(k_bimage / k_rowsum8 run at load time under every context.)

Every test prints one line with its worst error per leg (-s); profiles/NOTES.md keeps the figures."""
import numpy as np
import pytest

from rwkv_cpp_accelerated_amd import modelfile as mf
import chunk_cases as cc
import parity
from parity import TOL, _close

pytestmark = pytest.mark.gpu
STAGES = {"middle": (3, 1, 2), "first": (2, 0, 1), "last": (2, 1, 2)}          # kind -> n_layers, l0, l1
NAMES = "xy aa bb pp dd".split()
_T = {}


def _tensors(L, D):
    """one synthetic model at a time (a 5120-wide one is 2 GB of host memory): the parameter lists keep equal (L, D) next to each other"""
    if (L, D) not in _T:
        _T.clear()
        _T[(L, D)] = mf.synthetic_tensors(L, D, seed=6000 + D)
    return _T[(L, D)]


def _alias_xseq(m, D, buf):
    """the chunk path's residual buffer `buf` as a torch tensor [64][D] f64 (no copy), the way pipeline.EngineStage aliases x"""
    import torch

    class _X:
        __cuda_array_interface__ = dict(shape=(64, D), typestr="<f8", data=(m.xseq_device_ptr(buf), False), version=2)
    return torch.as_tensor(_X(), device="cuda:0")


def _update_leg(got, ref, x_in, what):
    """residual update of one row: |got - ref| <= TOL max |ref - x_in| + 2^-23 max |x_in|; returns the error relative to the update's max"""
    assert np.isfinite(got).all(), what
    upd = float(np.abs(ref - x_in).max()); d = float(np.abs(got - ref).max())
    cap = cc.update_eps(TOL, ref - x_in, x_in)
    assert d <= cap, f"{what}: max |d| = {d:.3e} > {TOL:.0e} max |update| + 2^-23 max |x_in| = {cap:.3e} (|update| {upd:.3e}, |x_in| {np.abs(x_in).max():.3e})"
    return d / max(upd, 1e-30)


def _tokens(n, seed):
    """n >= 3 ids with 0, VOCAB - 1 and one id that repeats within the chunk"""
    tk = [int(v) for v in np.random.default_rng(seed).integers(2, mf.VOCAB - 1, n)]
    tk[0], tk[-1] = 0, mf.VOCAB - 1
    tk[n // 2] = tk[n // 2 - 1] if n > 3 else tk[n // 2]
    if n > 3:
        assert len(set(tk)) == n - 1
    assert 0 in tk and mf.VOCAB - 1 in tk
    return tk


def _run_stage(oracle, kind, D, chunks, case_name="a", seed=1, row0=0):
    """One-layer stage context of `kind` at width D: state slot 0 planted from case `case_name`, then the chunks (row counts) one after
    the other on residual buffers 0, 1, 0, .. with the state carried over, each on freshly planted rows (first stage: token ids); every
    row and the state behind every chunk against the oracle, which continues from its own state.  Prints and returns the worst error per leg."""
    import torch
    from rwkv_cpp_accelerated_amd import engine
    L, l0, l1 = STAGES[kind]
    l, LD, V = l0, L * D, mf.VOCAB
    lo = slice(l * D, (l + 1) * D)
    case0 = cc.make_case(case_name, D, chunks[0], seed)
    t = cc.apply_ln2_mul(_tensors(L, D), L, D, l, case0.ln2_mul)
    ln = t[mf.LAYERNORMS].reshape(4 * (L + 1), D)
    m = engine.RWKV(resident=True)
    m.set_layer_range(l0, l1)
    m.loadTensors(L, D, t, maxGPT=64)
    om = oracle.from_tensors(L, D, t)
    xs = [_alias_xseq(m, D, 0), _alias_xseq(m, D, 1)]
    ref_state = cc.embed_state(case0.state, L, D, l, seed)
    for a, v in zip(m.state.arrays(), ref_state):
        a[:LD] = v
    pushed = [a[:LD].copy() for a in m.state.arrays()]
    m.push_state(1)
    worst = {}

    def note(k, e):
        worst[k] = max(worst.get(k, 0.0), e)

    for ci, n in enumerate(chunks):
        buf = ci & 1
        case = case0 if ci == 0 else cc.make_case(case_name, D, n, seed + ci)
        cc.check_case(case)
        assert np.array_equal(case.ln2_mul, case0.ln2_mul)
        assert row0 + n <= 64, f"row0 {row0} + n {n} does not fit the 64 logits rows"
        tag = f"{kind} stage [{l0},{l1}) of L={L} D={D} case {case_name} chunk {ci} n={n}"
        tokens = rows = None
        if kind == "first":
            tokens = _tokens(n, seed + ci)
        else:
            rows = case.rows
            xs[buf][:n].copy_(torch.from_numpy(rows))
            torch.cuda.synchronize()                                              # the engine runs on a stream of its own
        r0 = row0
        m.stage_chunk(tokens, n, row0=r0, buf=buf)
        m.sync()
        x_out = xs[buf][:n].cpu().numpy()
        m.pull_state(1)
        got_state = [a[:LD].copy() for a in m.state.arrays()]
        dd_prev = ref_state[4][lo].copy()
        ref = cc.oracle_stage_rows(oracle, om, t, L, D, l0, l1, rows, ref_state, tokens=tokens)
        if case_name == "g" and ci == 0:                                          # the case's claim at the width that runs here
            cc.check_case_g_tail(cc.hidden_sq(t, L, D, l, ref["x_mid"], dd_prev),
                                 cc.hidden_sq(t, L, D, l, ref["x_mid"], dd_prev, ln2_w=_tensors(L, D)[mf.LAYERNORMS].reshape(-1, D)[4 * l + 4]), tag)
        assert np.isfinite(ref["x_out"]).all() and all(np.isfinite(a).all() for a in ref_state), f"{tag}: the oracle's output is not finite"
        for i in range(n):
            note("update", _update_leg(x_out[i], ref["x_out"][i], ref["x_in"][i], f"{tag} row {i} leg update"))
        note("xy", _close(got_state[0][lo], ref_state[0][lo], f"{tag} leg state xy (ln1 of row {n - 1})"))
        note("aa", _close(got_state[1][lo], ref_state[1][lo], f"{tag} leg state aa", 1e-4))
        note("bb", _close(got_state[2][lo], ref_state[2][lo], f"{tag} leg state bb", 1e-4))
        if case_name == "f":
            e = float(np.abs(got_state[2][lo] / ref_state[2][lo] - 1.0).max())
            assert e <= 1e-4, f"{tag} leg state bb, element by element: {e:.3e} > 1e-4"
            note("bb/elem", e)
            e = cc.aa_elem_err(got_state[1][lo], ref_state[1][lo], ref["aa_mag"], ref["aa_vmax"], TOL / 1e-4)
            assert e <= 1e-4, f"{tag} leg state aa, element by element: {e:.3e} > 1e-4 of its terms' magnitudes (chunk_cases.aa_elem_err)"
            note("aa/elem", e)
        assert np.array_equal(got_state[3], pushed[3]), f"{tag} leg state pp: not what was pushed"
        xm, xi = ref["x_mid"][n - 1], ref["x_in"][n - 1]
        dd_cap = cc.ln_leg_bound(TOL, cc.update_eps(TOL, xm - xi, xi), xm, ln[4 * l + 4], ref_state[4][lo])
        note("dd", _close(got_state[4][lo], ref_state[4][lo], f"{tag} leg state dd (ln2 of row {n - 1}'s x_mid)", dd_cap))
        note("dd cap", dd_cap)
        for k in range(5):                                                        # the layers this context does not own
            for ll in range(L):
                if ll != l:
                    assert np.array_equal(got_state[k][ll * D: (ll + 1) * D], pushed[k][ll * D: (ll + 1) * D]), f"{tag}: state {NAMES[k]} of layer {ll} changed"
        if kind == "last":
            lg = m.logits(r0 + n).reshape(r0 + n, V)[r0:]
            for i in range(n):
                lno = oracle.layernorm(x_out[i][None, :], ln[4 * L + 2: 4 * L + 4])[0]
                lref = oracle.mm8_layer(lno, t[mf.HEAD], t[mf.HEADR], t[mf.HEADO], D, V, 0)
                note("logits", _close(lg[i], lref, f"{tag} row {i} leg logits (row {r0 + i})"))
    print(f"{kind} D={D} case {case_name} chunks {chunks} row0={row0}: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    om.close(); m.close()
    return worst


# chunk_cases.MIDDLE_RUNS: ten widths, at each one chunk of n <= 32 and one of n > 32 IN A ROW on one context: buffer 0, then buffer 1 from
# the state the first left (tests/test_chunk_cases_cpu.py checks that every row count of the set occurs in the list)
@pytest.mark.parametrize("D,chunks", cc.MIDDLE_RUNS)
def test_middle_stage_layer_on_planted_rows_and_state(built, oracle, D, chunks):
    _run_stage(oracle, "middle", D, chunks)


# cases b .. g at 1088 (17 k-blocks: 2 or 3 per octant) and 4160 (65: 8 or 9, the 10-k-block instances); the width varies slowest, so
# that the one synthetic model _tensors keeps is built once per width
@pytest.mark.parametrize("case_name", list("bcdefg"))
@pytest.mark.parametrize("D,chunks", [(1088, [17, 33]), (4160, [33])])
def test_middle_stage_layer_on_the_planted_cases(built, oracle, case_name, D, chunks):
    _run_stage(oracle, "middle", D, chunks, case_name=case_name, seed=3)


@pytest.mark.parametrize("D,chunks,case_name", [(128, [17, 33], "a"), (1088, [32, 47], "e"), (4096, [17, 33], "a")])
def test_first_stage_from_token_ids(built, oracle, D, chunks, case_name):
    """k_seq_embed + ln0 in front of layer 0: ids 0, VOCAB - 1 and a repeated id in every chunk; x_in of the update leg is the oracle's ln0"""
    _run_stage(oracle, "first", D, chunks, case_name=case_name, seed=5)


@pytest.mark.parametrize("D,chunks,row0", [(64, [32, 33], 0), (448, [17, 47], 5), (2048, [2, 64], 0), (5120, [17, 33], 3)])
def test_last_stage_and_its_logits_rows(built, oracle, D, chunks, row0):
    """ln_out + head behind the last layer: logits rows [row0, row0 + n) against the oracle's LayerNorm + head GEMV of the engine's own output rows"""
    w = _run_stage(oracle, "last", D, chunks, seed=7, row0=row0)
    assert "logits" in w


def _ln_cap(eps, x_ref, w, out_ref):
    return cc.ln_leg_bound(TOL, eps, x_ref, w, out_ref)


@pytest.mark.parametrize("D,N", [(448, 96), (1088, 2), (1088, 64), (4096, 33)])
def test_parralel_step_of_n_streams_on_planted_state(built, oracle, D, N):
    """The batched PARRALEL step (one token of N independent streams, stream s on state slot s) on an L = 2 model, every slot planted
    with different state, two rounds that continue from each other.  Reference: oracle_forward in mode 0.  Both layers' state of every
    slot with the module's bounds.  Those behind a vector that cannot be read back, per slot, from the oracle's own intermediate vectors
    (x0 = ln0(embedding row), x_mid0, x1 = layer 0's output, x_mid1) and the allowances eps of the updates in front of them:
        layer 0  xy: TOL (ln1 of x0)            dd: ln2 of x_mid0,  eps = TOL max |x_mid0 - x0| + ulp(x0)
        layer 1  xy: ln1 of x1, eps1 = TOL max |x1 - x0| + ulp(x0)      -- holds layer 0 AS A WHOLE to the tight bound
                 dd: ln2 of x_mid1, eps = eps1 + TOL max |x_mid1 - x1| + ulp(x1)
    each through chunk_cases.ln_leg_bound.  Logits by parity.check_logits; the two slots behind the N come back bit-equal."""
    from rwkv_cpp_accelerated_amd import engine
    L, V = 2, mf.VOCAB
    LD = L * D
    t = _tensors(L, D)
    ln = t[mf.LAYERNORMS].reshape(4 * (L + 1), D)
    emb = t[mf.EMBED].reshape(V, D)
    m = engine.RWKV(resident=True)
    m.loadTensors(L, D, t, maxGPT=N + 2)
    om = oracle.from_tensors(L, D, t)
    sp = cc.baseline_state(np.random.default_rng([9, D, N]), (N + 2) * LD)
    for a, v in zip(m.state.arrays(), sp):
        a[:] = v
    pushed = [a.copy() for a in sp]
    m.push_state(N + 2)
    worst = {}

    def note(k, e):
        worst[k] = max(worst.get(k, 0.0), e)

    for rnd in range(2):
        toks = [int(v) for v in np.random.default_rng([rnd, D, N]).integers(0, V, N)]
        toks[0], toks[-1] = 0, V - 1
        before = [a.copy() for a in sp]
        ref = om.forward(toks, sp, mode=0)
        got = m.forward(toks, engine.MODE_PARRALEL)[: N * V].reshape(N, V).copy()
        m.pull_state(N + 2)
        for s in range(N):
            tag = f"PARRALEL L={L} D={D} N={N} round {rnd} slot {s}"
            note("logits", parity.check_logits(got[s], ref[s], tag))
            sl = slice(s * LD, (s + 1) * LD)
            side = [a[sl].copy() for a in before]; whole = [a[sl].copy() for a in before]
            x0 = oracle.layernorm(emb[toks[s]].astype(np.float64)[None, :], ln[0:2])[0]
            x1 = np.zeros(D)
            om.stage_forward(toks[s], x1, 0, 1, whole)
            xm0 = cc.oracle_att_half(oracle, t, x0, side, 0, L, D)
            xm1 = cc.oracle_att_half(oracle, t, x1, side, 1, L, D)
            eps1 = cc.update_eps(TOL, x1 - x0, x0)
            caps = {(0, "xy"): TOL, (0, "dd"): _ln_cap(cc.update_eps(TOL, xm0 - x0, x0), xm0, ln[4], sp[4][sl][:D]),
                    (1, "xy"): _ln_cap(eps1, x1, ln[6], sp[0][sl][D:]),
                    (1, "dd"): _ln_cap(eps1 + cc.update_eps(TOL, xm1 - x1, x1), xm1, ln[8], sp[4][sl][D:])}
            for l in range(L):
                lo = slice(s * LD + l * D, s * LD + (l + 1) * D)
                st = m.state.arrays()
                note(f"xy{l}", _close(st[0][lo], sp[0][lo], f"{tag} layer {l} leg state xy", caps[(l, "xy")]))
                note(f"aa{l}", _close(st[1][lo], sp[1][lo], f"{tag} layer {l} leg state aa", 1e-4))
                note(f"bb{l}", _close(st[2][lo], sp[2][lo], f"{tag} layer {l} leg state bb", 1e-4))
                note(f"dd{l}", _close(st[4][lo], sp[4][lo], f"{tag} layer {l} leg state dd", caps[(l, "dd")]))
                note(f"cap xy{l}", caps[(l, "xy")]); note(f"cap dd{l}", caps[(l, "dd")])
        for k, a in enumerate(m.state.arrays()):
            assert np.array_equal(a[N * LD: (N + 2) * LD], pushed[k][N * LD:]), f"PARRALEL D={D} N={N} round {rnd}: state {NAMES[k]} of a slot >= N changed"
        assert np.array_equal(m.state.arrays()[3][: N * LD], pushed[3][: N * LD]), f"PARRALEL D={D} N={N} round {rnd}: state pp"
    print(f"PARRALEL D={D} N={N}: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    om.close(); m.close()
