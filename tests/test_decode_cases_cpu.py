"""The planted cases on the decode kernels (tests/decode_cases.py), without a GPU: the planting recipe, passed through the oracle's LayerNorm,
yields a residual vector that keeps the case's claim, and the ORACLE'S PIECE of every decode launch stays within HALF of that launch's GPU
bound (tests/test_kernels_gpu.py) of the plain f64 evaluation of the same launch on the same input -- the pattern of
tests/test_chunk_cases_cpu.py.  That half is what lets the GPU suite hold k_att, k_ffn_rk and k_head to TOL of f64 directly (its f64 legs) with no
new number, and what makes a failure of an oracle leg there attributable to the engine.

The walk is the oracle's own token: x = ln0(embedding row), then per launch the oracle's piece and the f64 evaluation, both on the ORACLE'S x and
state, the oracle's result carried forward; at the end the walk's residual vector, state and logits are bit-equal to oracle_stage_forward's
(chunk_cases.oracle_stage_rows with l0 = 0 from the tokens), so the pieces ARE the stage.  Legs and caps:
  first x, att y (times the att_out scale), xy, sigmoid(r), relu(k)^2 (times the ffn_v scale), dd, logits     TOL / 2 of the vector's max
  att aa, bb                                                                                                  1e-4 / 2 (case f: also per element)
  the two residual updates                       half of chunk_cases.update_eps: TOL / 2 of the update's max plus half an f32 ulp at max |x|

Measured (two tokens, case b one per magnitude; L = 2 at 1040, L = 1 at 4096 as on the GPU; worst leg as a FRACTION OF ITS CAP; the log of the
run is profiles/decode_cases/oracle_vs_f64_cpu.log) -- no constant of chunk_cases.py had to be reduced for the decode variant:
  residual update behind att_out   0.61 (case e, 1040), 0.52 / 0.46 (case c, 1040 / 4096), 0.44 (g), 0.26 / 0.17 (b+), <= 0.12 elsewhere
  residual update behind ffn_v     0.24 (case c, 4096), <= 0.08 elsewhere
  relu(k)^2, sigmoid(r), y, logits 0.27, 0.16, 0.14, 0.14 (case c, 4096); <= 0.09 elsewhere
  aa, bb                           0.06, 0.02 (case c, 4096); case f element by element 0.01, 0.01
  first x, xy, dd                  0.02, 0.10, 0.13 (case c, 4096)
Case c is the worst of most legs for the reason chunk_cases.py gives (the reference's f32 LayerNorm mean); the att_out update is the leg with the
least room everywhere, as in the chunk suite (the reference's 17 f32 roundings at the magnitude of x, chunk_cases.py)."""
import numpy as np
import pytest

from rwkv_cpp_accelerated_amd import modelfile as mf
import chunk_cases as cc
import decode_cases as dcs
from parity import TOL

_T = {}


def _tensors(L, D):
    if (L, D) not in _T:
        _T.clear()
        _T[(L, D)] = mf.synthetic_tensors(L, D, seed=4000 + D)
    return _T[(L, D)]


NAMES = ["a", "b-", "b+", "c", "d", "e", "f", "g"]


# (width, layers) as the GPU suite runs them: two layers at 1040, where layer 1's k_att consumes a site opened by k_ffnv on the planted residual
# plus layer 0's updates; one at 4096
@pytest.mark.parametrize("name,D,L", [(c, 1040, 2) for c in NAMES] + [(c, 4096, 1) for c in ("b-", "b+", "c", "d")])
def test_planted_case_keeps_its_claim_and_the_oracle_pieces_stay_within_half_of_each_leg_of_f64(oracle, name, D, L):
    dc = dcs.decode_case(name, D, L)
    case = dc.case
    n = case.rows.shape[0]
    toks = list(dcs.TOKENS[:n])
    half = 0.5 * TOL
    frac = {}                                                                 # leg -> worst error as a fraction of its cap

    def leg(k, err, cap):
        frac[k] = max(frac.get(k, 0.0), err / cap)

    with dcs.planted(_tensors(L, D), L, D, case.rows, ln2_mul=case.ln2_mul) as t:
        ln = t[mf.LAYERNORMS].reshape(4 * (L + 1), D)
        emb = t[mf.EMBED].reshape(mf.VOCAB, D)[toks].astype(np.float64)
        cc.check_state(case, [a[:D] for a in dc.state])
        st = [a.copy() for a in dc.state]                                     # the walk's state: the oracle's
        st_stage = [a.copy() for a in dc.state]
        om = oracle.from_tensors(L, D, t)
        o = cc.oracle_stage_rows(oracle, om, t, L, D, 0, L, None, st_stage, tokens=toks, want_logits=True)
        om.close()
        gtail = dcs.GTail(_tensors(L, D)[mf.LAYERNORMS].reshape(-1, D)[4])
        for i in range(n):
            x = oracle.layernorm(emb[i][None, :], ln[0:2])[0]
            dcs.check_planted(dc, i, x)
            leg("first x", dcs.rel(x, cc._ln(emb[i], ln[0], ln[1])), half)
            for l in range(L):
                lo = slice(l * D, (l + 1) * D)
                # k_att
                oa, fa = dcs.oracle_att(oracle, t, L, D, l, x, st), dcs.f64_att(t, L, D, l, x, st)
                sc = t[mf.ATTOUTR][lo].astype(np.float64)
                leg("att y", dcs.rel(oa["y"].astype(np.float32) * t[mf.ATTOUTR][lo], fa["ybuf"]), half)
                leg("att aa", dcs.rel(oa["aa"], fa["aa"]), 0.5e-4)
                leg("att bb", dcs.rel(oa["bb"], fa["bb"]), 0.5e-4)
                if name == "f":
                    mag, vmax = dcs.aa_scales(t, D, l, st[1][lo], oa["k"], oa["v"])
                    leg("att aa/elem", cc.aa_elem_err(oa["aa"], fa["aa"], mag, vmax, TOL / 1e-4), 0.5e-4)
                    leg("att bb/elem", float(np.abs(oa["bb"] / fa["bb"] - 1.0).max()), 0.5e-4)
                leg("attout xy", dcs.rel(oa["ln1"], cc._ln(x, ln[4 * l + 2], ln[4 * l + 3])), half)
                # k_attout
                x1 = dcs.oracle_attout(oracle, t, L, D, l, x, oa["y"])
                upd = dcs.matvec64(fa["ybuf"] / sc, t, mf.ATTOUT, mf.ATTOUTR, mf.ATTOUTO, l, D, D)
                leg("attout x", dcs.update_err(x1 - x, upd, x, TOL), 0.5)
                st[0][lo], st[1][lo], st[2][lo] = oa["ln1"], oa["aa"], oa["bb"]
                # k_ffn_rk
                of, ff = dcs.oracle_ffn_rk(oracle, t, L, D, l, x1, st), dcs.f64_ffn_rk(t, L, D, l, x1, st)
                leg("ffn sigmoid(r)", dcs.rel(of["sig"], ff["sig"]), half)
                leg("ffn relu^2(k)", dcs.rel(of["h"] * t[mf.FFNVR][l * 4 * D: (l + 1) * 4 * D], ff["hbuf"]), half)
                leg("ffnv dd", dcs.rel(of["ln2"], cc._ln(x1, ln[4 * l + 4], ln[4 * l + 5])), half)
                if name == "g" and l == 0:
                    gtail.check(t, L, D, x1, st, ff, f"case g D={D} token {i}")
                # k_ffnv
                x = dcs.oracle_ffnv(oracle, t, L, D, l, x1, of["h"], of["sig"])
                upd = dcs.matvec64(ff["h"], t, mf.FFNV, mf.FFNVR, mf.FFNVO, l, 4 * D, D) * ff["sig"]
                leg("ffnv x", dcs.update_err(x - x1, upd, x1, TOL), 0.5)
                st[4][lo] = of["ln2"]
            # k_head
            lg = dcs.oracle_head(oracle, t, L, D, x)
            leg("head", dcs.rel(lg, dcs.f64_head(t, L, D, x)), half)
            assert np.array_equal(x, o["x_out"][i]) and np.array_equal(lg, o["logits"][i]), f"case {name} D={D} token {i}: the pieces are not oracle_stage_forward"
        assert all(np.array_equal(a, b) for a, b in zip(st, st_stage)), f"case {name} D={D}: the pieces' state is not oracle_stage_forward's"
    print(f"case {name} D={D} L={L} n={n} oracle pieces vs f64, fraction of each leg's cap: " + ", ".join(f"{k} {v:.2f}" for k, v in frac.items()))
    bad = {k: v for k, v in frac.items() if not v <= 1.0}
    assert not bad, f"case {name} D={D}: the oracle is outside half the GPU bound of f64 on {bad}"


def test_planting_restores_the_embedding_rows_and_leaves_the_model_alone():
    """decode_cases.planted changes the cached model's embedding rows in place: behind the block they, and every other tensor, are what they were"""
    L, D = 1, 1040
    t = _tensors(L, D)
    before = [None if a is None else a.copy() for a in t]
    rows = np.random.default_rng(1).standard_normal((2, D)) * 3.0 + 5.0
    with dcs.planted(t, L, D, rows, ln2_mul=np.full(D, 2.0)) as tt:
        emb = tt[mf.EMBED].reshape(mf.VOCAB, D)
        assert np.array_equal(emb[list(dcs.TOKENS)], rows.astype(np.float32))
        x = cc._ln(emb[list(dcs.TOKENS)].astype(np.float64), *tt[mf.LAYERNORMS].reshape(-1, D)[0:2])
        assert np.abs(x[0] - rows[0]).max() <= 1e-5 * np.abs(rows[0]).max()
    assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(t, before))


@pytest.mark.parametrize("which,D", [("h", 1040), ("t", 1040), ("h", 4096), ("t", 4096)])
def test_cases_h_and_t_keep_their_claims_and_the_derived_bound_holds_for_the_restated_arithmetic(which, D):
    """Cases h and t (decode_cases.case_h / case_t) without a GPU: the claim (h: the scale bound is >= 100 x max |v_m|; t: max |v_k| is >= 0.99 of
    it, on the channel of the largest |C_k|), site_vectors / site_bound agree with f64_att, and k_att's arithmetic restated in numpy with its
    roundings (decode_cases.emulate_att) stays inside the derived bounds -- the extremes of the formats included: case t has gates of 1e-75, below
    an f32.  And the bound is not vacuous: the same arithmetic with a scale 1 % too small wraps case t's largest element and lands far outside."""
    L = 1
    t0 = _tensors(L, D)
    dc = dcs.case_h(D, L) if which == "h" else dcs.case_t(t0, L, D)
    with dcs.planted(t0, L, D, dc.case.rows, ln0_bias=0.0 if which == "t" else None) as t:
        ln = t[mf.LAYERNORMS].reshape(4 * (L + 1), D)
        x = cc._ln(t[mf.EMBED].reshape(mf.VOCAB, D)[dcs.TOKENS[0]].astype(np.float64), ln[0], ln[1])
        sv = dcs.site_vectors(t, L, D, 0, "att", x, dc.state[0][:D])
        if which == "h":
            assert all(s["amax"] >= 100.0 * s["true"] for s in sv)
        else:
            j = dc.case.claims["channel"]
            assert j == int(np.argmax(np.abs(sv[0]["C"]))) == int(np.argmax(np.abs(sv[0]["B"]))) == int(np.argmax(np.abs(x - x.mean())))
            assert sv[0]["true"] >= 0.99 * sv[0]["amax"]
        fa = dcs.f64_att(t, L, D, 0, x, dc.state)
        outs = [dcs.site_bound(t, 0, D, s) for s in sv]
        for (exact, _), key in zip(outs, "kvr"):
            assert np.allclose(exact, fa[key], rtol=0.0, atol=1e-9 * np.abs(fa[key]).max())
        b = dcs.att_bound(t, D, 0, fa, dc.state, *(o[1] for o in outs))
        em = dcs.emulate_att(t, D, 0, x, dc.state, sv)
        ratios = {k: dcs.bound_ratio(em[k], fa[k], b[k]) for k in ("ybuf", "aa", "bb")}
        print(f"case {which} D={D} restated arithmetic, measured / bound: {ratios}, largest |q| {em['qmax']:.0f} of {dcs.QLIM:.0f}")
        assert em["qmax"] <= dcs.QLIM + 2 and all(v <= 1.0 for v in ratios.values()), ratios
        if which == "t":
            bad = dcs.emulate_att(t, D, 0, x, dc.state, sv, amax_factor=0.99)
            assert bad["qmax"] > 2.0 ** 22 and dcs.bound_ratio(bad["ybuf"], fa["ybuf"], b["ybuf"]) > 10.0
