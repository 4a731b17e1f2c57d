"""The planted cases of the chunk-path layer tests (tests/chunk_cases.py), without a GPU: every case has the property it claims, the
oracle's output on it is finite, and the ORACLE ALONE stays within half of each leg's tolerance of a plain f64 numpy evaluation of the
same layer (chunk_cases.f64_stage: u r + o dequantised per input row, every product and sum in f64, the same stage formulae).  That
half is what makes a failure of tests/test_chunk_layers_gpu.py attributable to the engine: where the reference's own f32 arithmetic
(the f32 mean of its LayerNorm, its f32 GEMV partial sums, its f32 k in front of exp) used up the tolerance, a correct engine -- which
keeps f64 where the reference rounds -- could fail, and a wrong one could hide.  A case that broke the cap had its ratio or span
reduced in chunk_cases.py until the oracle held (OFFSET_C, TOP_B, REST_D: see there); the cap does not move."""
import numpy as np
import pytest

from rwkv_cpp_accelerated_amd import modelfile as mf
import chunk_cases as cc
from parity import TOL

_T = {}


def _tensors(L, D):
    if (L, D) not in _T:
        _T.clear()
        _T[(L, D)] = mf.synthetic_tensors(L, D, seed=6000 + D)
    return _T[(L, D)]


def _rel(got, ref, extra=0.0):
    """the tol at which got is just inside tol max |ref| + extra of ref"""
    d = float(np.abs(np.asarray(got, np.float64) - ref).max())
    return max(d - extra, 0.0) / max(float(np.abs(ref).max()), 1e-30)


# every case at 128 (two k-blocks: six empty octants) and 448 (KB = 7); the three whose values were reduced (chunk_cases.py) also at the
# wide width the GPU suite runs them at -- the reference's f32 mean loses more over 4160 channels than over 448
@pytest.mark.parametrize("name,D,n", [(c, D, n) for D, n in ((128, 33), (448, 17)) for c in cc.CASES] + [(c, 4160, 17) for c in "bcd"])
def test_case_keeps_its_claim_and_the_oracle_stays_within_half_the_tolerance_of_f64(oracle, name, D, n):
    """Middle stage [1, 2) of L = 3 on the planted rows and state.  Legs and caps (half of what the GPU suite allows the engine):
    residual update per row TOL / 2 of its max plus HALF an f32 ulp of the accumulator; state xy TOL / 2; aa, bb 1e-4 / 2 (case f: also
    element by element, as on the GPU); dd TOL / 2 plus half the update's allowance through ln2 (chunk_cases.ln_leg_bound).  And the
    att_out half the GPU suite's dd and PARRALEL caps are computed from (chunk_cases.oracle_att_half) is oracle_stage_forward's: ln2 of
    its last row is bit-equal to the dd state the stage left."""
    L, l = 3, 1
    case = cc.make_case(name, D, n, seed=11)
    cc.check_case(case)
    t = cc.apply_ln2_mul(_tensors(L, D), L, D, l, case.ln2_mul)
    ln = t[mf.LAYERNORMS].reshape(4 * (L + 1), D)
    st_o = cc.embed_state(case.state, L, D, l, seed=11)
    st_f = [a.copy() for a in st_o]
    om = oracle.from_tensors(L, D, t)
    o = cc.oracle_stage_rows(oracle, om, t, L, D, l, l + 1, case.rows, st_o)
    om.close()
    f = cc.f64_stage(t, L, D, l, l + 1, case.rows, st_f)
    assert np.isfinite(o["x_out"]).all() and all(np.isfinite(a).all() for a in st_o), f"case {name} D={D}: the oracle's output is not finite"
    assert np.isfinite(f["x_out"]).all() and all(np.isfinite(a).all() for a in st_f)
    if name == "g":
        dd0 = case.state[4]
        h = cc.hidden_sq(t, L, D, l, f["x_mid"], dd0)
        assert np.allclose(h, f["h"], rtol=1e-12, atol=0.0)                       # the helper the GPU suite measures the claim with
        cc.check_case_g_tail(h, cc.hidden_sq(t, L, D, l, f["x_mid"], dd0, ln2_w=_tensors(L, D)[mf.LAYERNORMS].reshape(-1, D)[4 * l + 4]), f"case g D={D}")
    half = 0.5 * TOL
    lo = slice(l * D, (l + 1) * D)
    worst = {}
    for i in range(n):
        xin = case.rows[i]
        e = _rel(o["x_out"][i] - xin, f["x_out"][i] - xin, 0.5 * cc.ULP32 * np.abs(xin).max())
        worst["update"] = max(worst.get("update", 0.0), e)
        assert e <= half, f"case {name} D={D} n={n} row {i}: oracle's residual update is {e:.2e} of its max from f64 (> {half:.1e})"
    worst["xy"] = _rel(st_o[0][lo], st_f[0][lo])
    worst["aa"] = _rel(st_o[1][lo], st_f[1][lo])
    worst["bb"] = _rel(st_o[2][lo], st_f[2][lo])
    worst["dd"] = _rel(st_o[4][lo], st_f[4][lo])
    assert np.array_equal(oracle.layernorm(o["x_mid"][n - 1][None, :], ln[4 * l + 4: 4 * l + 6])[0], st_o[4][lo]), \
        f"case {name} D={D}: chunk_cases.oracle_att_half is not the att_out half of oracle_stage_forward"
    if name == "f":
        worst["bb/elem"] = float(np.abs(st_o[2][lo] / st_f[2][lo] - 1.0).max())
        worst["aa/elem"] = cc.aa_elem_err(st_o[1][lo], st_f[1][lo], o["aa_mag"], o["aa_vmax"], TOL / 1e-4)
        assert worst["bb/elem"] <= 0.5e-4 and worst["aa/elem"] <= 0.5e-4, f"case f D={D}: element by element bb {worst['bb/elem']:.2e} aa {worst['aa/elem']:.2e}"
    xm = f["x_mid"][n - 1]
    dd_cap = cc.ln_leg_bound(half, 0.5 * cc.update_eps(TOL, xm - case.rows[n - 1], case.rows[n - 1]), xm, ln[4 * l + 4], st_f[4][lo])
    print(f"case {name} D={D} n={n} oracle vs f64: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()) + f" (dd cap {dd_cap:.1e})")
    assert worst["xy"] <= half, f"case {name} D={D}: state xy {worst['xy']:.2e}"
    assert worst["aa"] <= 0.5e-4 and worst["bb"] <= 0.5e-4, f"case {name} D={D}: state aa {worst['aa']:.2e} bb {worst['bb']:.2e}"
    assert worst["dd"] <= dd_cap, f"case {name} D={D}: state dd {worst['dd']:.2e} > {dd_cap:.2e}"
    assert np.array_equal(st_o[3], st_f[3]), "pp is carried through"


def test_first_and_last_stage_of_the_f64_evaluation_follow_the_oracle(oracle):
    """the embedding + ln0 entry and the ln_out + head exit of chunk_cases.f64_stage against oracle_stage_forward (ids 0, VOCAB - 1 and
    a repeated one), so that the evaluation is usable for every stage kind the GPU suite runs"""
    L, D = 2, 128
    t = _tensors(L, D)
    toks = [0, mf.VOCAB - 1, 4242, 4242, 17]
    rng = np.random.default_rng(5)
    st_o = cc.baseline_state(rng, L * D); st_f = [a.copy() for a in st_o]
    om = oracle.from_tensors(L, D, t)
    o0 = cc.oracle_stage_rows(oracle, om, t, L, D, 0, 1, None, st_o, tokens=toks)
    o1 = cc.oracle_stage_rows(oracle, om, t, L, D, 1, 2, o0["x_out"], st_o, want_logits=True)
    om.close()
    f0 = cc.f64_stage(t, L, D, 0, 1, None, st_f, tokens=toks)
    f1 = cc.f64_stage(t, L, D, 1, 2, o0["x_out"], st_f, want_logits=True)
    assert _rel(o0["x_in"], f0["x_in"]) <= 0.5 * TOL
    for i in range(len(toks)):
        assert _rel(o0["x_out"][i] - o0["x_in"][i], f0["x_out"][i] - f0["x_in"][i], 0.5 * cc.ULP32 * np.abs(o0["x_in"][i]).max()) <= 0.5 * TOL, i
        assert _rel(o1["logits"][i], f1["logits"][i]) <= 0.5 * TOL, i


def test_middle_stage_runs_cover_the_widths_and_row_counts():
    """the GPU suite's middle-stage list: ten widths, each with one chunk of n <= 32 and one of n > 32, every row count of the set
    somewhere -- a width dropped from the list must not drop a row count with it"""
    assert [D for D, _ in cc.MIDDLE_RUNS] == [64, 128, 448, 1088, 1536, 2048, 4096, 4160, 5056, 5120]
    assert {n for _, ch in cc.MIDDLE_RUNS for n in ch} == cc.ROW_COUNTS == {1, 2, 17, 32, 33, 47, 64}
    assert all(len(ch) == 2 and ch[0] <= 32 < ch[1] for _, ch in cc.MIDDLE_RUNS)


def test_ln_leg_bound_covers_a_perturbed_layernorm():
    """the derivation in chunk_cases.ln_leg_bound, numerically: LayerNorm of x + e with |e| <= eps (random signs, and the two worst
    directions: along x - mean and one element alone) stays inside the bound, and the bound is not slack by more than a small factor"""
    rng = np.random.default_rng(3)
    for D in (64, 1088):
        x = rng.standard_normal(D) * 3.0 + 1.0; w = 1.0 + 0.1 * rng.standard_normal(D); b = 0.1 * rng.standard_normal(D)
        out = cc._ln(x, w, b)
        eps = 1e-4
        bound = cc.ln_leg_bound(0.0, eps, x, w, out)
        worst = 0.0
        es = [eps * rng.choice([-1.0, 1.0], D) for _ in range(50)] + [eps * np.sign(x - x.mean()), -eps * np.sign(x - x.mean())]
        one = np.zeros(D); one[int(np.argmax(np.abs(x - x.mean())))] = eps
        for e in es + [one, -one]:
            worst = max(worst, float(np.abs(cc._ln(x + e, w, b) - out).max()) / float(np.abs(out).max()))
        assert worst <= bound, (D, worst, bound)
        assert worst >= bound / 8.0, (D, worst, bound)
