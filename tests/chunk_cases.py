"""Planted inputs of the chunk-path layer tests (tests/test_chunk_layers_gpu.py on the GPU, tests/test_chunk_cases_cpu.py without one),
the bound of a state leg that sits one LayerNorm behind a vector nobody can read back, and a plain f64 numpy evaluation of a layer
range that tells the oracle's own error from the engine's.  TEST INFRASTRUCTURE: nothing here is imported by the product.

A case is a pure function of (D, n, seed): rows [n][D] f64 (the residual stream handed to the layer), the five state vectors of that
layer ([D] each: xy, aa, bb, pp, dd), a multiplier [D] on the layer's ln2 weight row (ones except in case g), and `claims`, the
measured properties the case exists for.  `check_case` asserts them on the input that was built, so that a case cannot degenerate
without a test failing.  Zero-variance rows are never produced (the reference's LayerNorm has no epsilon: it would divide by zero).

  a  baseline: rows N(0, 1); xy, dd, aa, pp N(0, 1), bb U(0.5, 2) -- the state distribution of tests/test_kernels_gpu.py
  b  row magnitudes six decades apart within one chunk                       (scales and statistics are per token)
  c  a common offset OFFSET_C on every channel                                (the f64 subtraction of the mean)
  d  N_OUT outlier channels at OUTLIER_D x the rest, inside ONE 64-channel k-block  (per-octant scale and cA record)
  e  xy and dd state with outliers above any LayerNorm output                (a caller may set any state: setSubState)
  f  bb over +-SPAN_F decades, aa = bb N(0, 1): aa and bb both span them, bb > 0
  g  ln2 weights HOT_G x on a few channels: relu(k)^2 heavy-tailed over the 4 D hidden units

Values that were REDUCED until the oracle held the cap of tests/test_chunk_cases_cpu.py (within half of each leg's tolerance of the
f64 evaluation below); the cap did not move.  Two properties of the REFERENCE, which the oracle restates, are behind all three:
  * it pre-loads the att_out accumulator with f32(x) and adds the GEMV's 16 slab partial sums to it one by one (rwkv.cu:267-295, :548):
    17 roundings at the magnitude of x, about 2 ulp(max |x|) from the exact sum, where the update leg grants one.  The excess stays
    under TOL / 2 of an update of ~0.3 only while max |x| is below ~25;
  * it accumulates the LayerNorm mean in f32 (rwkv.cu:412-444): at a common offset c the mean is off by some 1e-7 c sqrt(D / 16),
    which a unit-variance row hands to the LayerNorm output undiminished.
 OFFSET_C  asked for: about 1e3.  At 1e3 the oracle is 1e-4 from f64 (both effects); at 10 its update is 8.5e-6 .. 1.3e-5 of 1.5e-5 at the widths
           128, 448 and 4160, with half an ulp of the accumulator granted beside it (30 would be 2.7e-5).  The mean is still 10 standard deviations from zero: a one-pass f32 variance fails there.
 TOP_B     the six decades of case b are 10^-5.5 .. 10^0.5 instead of 10^-3 .. 10^3: rows of magnitude 1e2 and up were 2.9e-5 .. 1e-3 off.
 REST_D    case d keeps its ratio of 100 with the outliers at 3 and the rest at 0.03 (outliers at 100: 2.6e-5)."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from rwkv_cpp_accelerated_amd import modelfile as mf

CASES = "abcdefg"
OFFSET_C = 10.0
TOP_B = 0.5
OUTLIER_D, N_OUT, REST_D = 100.0, 3, 0.03
OUTLIER_E = 200.0
SPAN_F = 20.0
HOT_G, FRAC_G = 30.0, 0.05
ULP32 = 2.0 ** -23


# The middle-stage runs of the GPU suite: (width, [n <= 32, n > 32]).  Widths, all multiples of 64: 64 has seven empty octants; 448 is
# KB = 7; 1536 the narrowest width with k_seq_gemm_b; 4160 the first with the 10-k-block instances.  Each width runs one chunk of n <= 32
# and one of n > 32 (two 32-row halves) IN A ROW on one context.  Over the list every n of ROW_COUNTS occurs (checked without a GPU).
ROW_COUNTS = {1, 2, 17, 32, 33, 47, 64}
MIDDLE_RUNS = [(64, [17, 47]), (128, [2, 33]), (448, [32, 64]), (1088, [1, 47]), (1536, [17, 64]), (2048, [32, 33]),
               (4096, [2, 64]), (4160, [17, 33]), (5056, [1, 47]), (5120, [32, 64])]


@dataclass
class Case:
    name: str
    rows: np.ndarray
    state: list                      # xy, aa, bb, pp, dd: [D] each
    ln2_mul: np.ndarray
    claims: dict = field(default_factory=dict)


def baseline_state(rng, n):
    """the distribution tests/test_kernels_gpu.py plants: every mix / WKV term sees real numbers; returns xy, aa, bb, pp, dd"""
    xy = rng.standard_normal(n); dd = rng.standard_normal(n)
    aa = rng.standard_normal(n); bb = 0.5 + 1.5 * rng.random(n); pp = rng.standard_normal(n)
    return [xy, aa, bb, pp, dd]


def make_case(name: str, D: int, n: int, seed: int) -> Case:
    rng = np.random.default_rng([seed, D, n, CASES.index(name)])
    rows = rng.standard_normal((n, D))
    xy, aa, bb, pp, dd = baseline_state(rng, D)
    mul = np.ones(D)
    claims = {}
    if name == "b":
        mag = 10.0 ** np.linspace(TOP_B - 6.0, TOP_B, n) if n > 1 else np.ones(1)
        rows *= rng.permutation(mag)[:, None]
        rms = np.sqrt((rows ** 2).mean(axis=1))
        claims["row_rms_ratio"] = float(rms.max() / rms.min())
    elif name == "c":
        rows += OFFSET_C
        claims["mean_over_std"] = float(np.abs(rows.mean(axis=1) / rows.std(axis=1)).min())
    elif name == "d":
        kb = min(1, D // 64 - 1)                                      # the second k-block where there is one
        ch = 64 * kb + rng.choice(64, N_OUT, replace=False)
        rows *= REST_D
        rows[:, ch] = REST_D * OUTLIER_D * rng.choice([-1.0, 1.0], (n, N_OUT)) * (1.0 + 0.1 * rng.random((n, N_OUT)))
        rest = np.delete(rows, ch, axis=1)
        claims["k_blocks"] = sorted(set(int(c) // 64 for c in ch))
        claims["channels"] = sorted(int(c) for c in ch)
        claims["outlier_over_rest_rms"] = float((np.abs(rows[:, ch]).min(axis=1) / np.sqrt((rest ** 2).mean(axis=1))).min())
    elif name == "e":
        for v in (xy, dd):
            ch = rng.choice(D, 4, replace=False)
            v[ch] = OUTLIER_E * rng.choice([-1.0, 1.0], 4)
        claims["state_max"] = float(min(np.abs(xy).max(), np.abs(dd).max()))
        claims["ln_output_cap"] = float(np.sqrt(D - 1.0) * 1.5 + 0.5)     # |w| <= 1.5, |b| <= 0.5 in the synthetic models; |z| <= sqrt(D - 1)
    elif name == "f":
        bb = 10.0 ** rng.uniform(-SPAN_F, SPAN_F, D)
        bb[:2] = 10.0 ** np.array([-SPAN_F, SPAN_F])                  # both ends are there at every width
        aa = bb * rng.standard_normal(D)
        claims["bb_decades"] = float(np.log10(bb.max() / bb.min()))
        claims["aa_decades"] = float(np.log10(np.abs(aa).max() / np.abs(aa).min()))
        claims["bb_min"] = float(bb.min())
    elif name == "g":
        rm = np.random.default_rng([D, 7])                            # the MODEL's part of the case: the same for every n and seed
        hot = rm.random(D) < FRAC_G
        hot[rm.choice(D, 2, replace=False)] = True
        mul[hot] = HOT_G
        claims["hot_channels"] = int(hot.sum())
        claims["hot_ratio"] = float(mul.max() / mul.min())
    elif name != "a":
        raise ValueError(name)
    return Case(name, rows, [xy, aa, bb, pp, dd], mul, claims)


def check_case(c: Case):
    """the property each case claims, on the input it built"""
    n, D = c.rows.shape
    assert np.isfinite(c.rows).all() and all(np.isfinite(s).all() for s in c.state), c.name
    assert (c.rows.std(axis=1) > 0).all(), f"case {c.name}: zero-variance row"
    assert (c.state[2] > 0).all(), f"case {c.name}: bb <= 0"
    k = c.claims
    if c.name == "b":
        assert n < 2 or k["row_rms_ratio"] >= 0.9e6, k
    elif c.name == "c":
        assert k["mean_over_std"] >= 0.5 * OFFSET_C, k
    elif c.name == "d":
        assert len(k["k_blocks"]) == 1 and k["outlier_over_rest_rms"] >= 0.75 * OUTLIER_D, k
    elif c.name == "e":
        assert k["state_max"] >= OUTLIER_E > k["ln_output_cap"], k
    elif c.name == "f":
        assert k["bb_decades"] >= 2 * SPAN_F - 1e-9 and k["aa_decades"] >= 2 * SPAN_F - 2 and k["bb_min"] > 0, k
    elif c.name == "g":
        assert 2 <= k["hot_channels"] <= max(2, D // 8) and k["hot_ratio"] == HOT_G, k


def check_rows(c: Case, x):
    """the claims of case c that are made on its ROWS, measured again on x [n][D]: the vectors a kernel was actually handed (read back
    behind k_first in tests/test_kernels_gpu.py, or the oracle's ln0 output), which are not bit-equal to c.rows"""
    x = np.asarray(x, np.float64)
    assert np.isfinite(x).all() and (x.std(axis=1) > 0).all(), c.name
    if c.name == "c":
        m = float(np.abs(x.mean(axis=1) / x.std(axis=1)).min())
        assert m >= 0.5 * OFFSET_C, f"case c: |mean| / std = {m:.3g} on the planted vector"
    elif c.name == "d":
        ch = c.claims["channels"]
        rest = np.delete(x, ch, axis=1)
        m = float((np.abs(x[:, ch]).min(axis=1) / np.sqrt((rest ** 2).mean(axis=1))).min())
        assert len(c.claims["k_blocks"]) == 1 and m >= 0.75 * OUTLIER_D, f"case d: outlier / rms of the rest = {m:.3g} on the planted vector"


def check_state(c: Case, state):
    """the claims of case c that are made on its STATE, measured again on the five [D] vectors a context was handed"""
    xy, aa, bb, pp, dd = (np.asarray(a, np.float64) for a in state)
    assert all(np.isfinite(a).all() for a in (xy, aa, bb, pp, dd)) and (bb > 0).all(), c.name
    if c.name == "e":
        assert min(np.abs(xy).max(), np.abs(dd).max()) >= OUTLIER_E > c.claims["ln_output_cap"], "case e: the pushed xy / dd state lost its outliers"
    elif c.name == "f":
        assert np.log10(bb.max() / bb.min()) >= 2 * SPAN_F - 1e-9 and np.log10(np.abs(aa).max() / np.abs(aa).min()) >= 2 * SPAN_F - 2, \
            "case f: the pushed aa / bb state lost its span"


def apply_ln2_mul(t, L, D, layer, mul):
    """the model's tensor list with ln2's weight row of `layer` multiplied by mul (a new list; `t` is not changed)"""
    if np.all(mul == 1.0):
        return t
    t = list(t)
    ln = t[mf.LAYERNORMS].reshape(4 * (L + 1), D).copy()
    ln[4 * layer + 4] = (ln[4 * layer + 4] * mul).astype(np.float32).astype(np.float64)
    t[mf.LAYERNORMS] = ln.reshape(-1)
    return t


def embed_state(case_state, L, D, layer, seed):
    """whole [L][D] state arrays: the case's vectors in `layer`, the baseline in the others"""
    full = baseline_state(np.random.default_rng([seed, L, D]), L * D)
    for a, v in zip(full, case_state):
        a[layer * D: (layer + 1) * D] = v
    return full


# ---- bounds -----------------------------------------------------------------------------------------------------------------
def update_eps(tol, upd_ref, x_in):
    """allowed absolute error of a residual vector behind an update: tol of the update's max, plus one f32 ulp at max |x_in| -- the
    reference rounds f32(x) + att_out . y to f32 (rwkv.cu:548-553), two correct implementations may differ by that ulp"""
    return tol * float(np.abs(upd_ref).max()) + ULP32 * float(np.abs(x_in).max())


def ln_leg_bound(tol, eps, x_ref, w, out_ref):
    """Bound (relative to max |out_ref|) of a leg out = w (x - mean) / sd + b whose input x cannot be read back and is only known to
    lie within eps (absolute, per element) of x_ref.  With e = x - x_ref, |e_i| <= eps, z = (x_ref - mean) / sd and the unbiased sd over
    D elements, to first order in eps / sd:
        d out_i = w_i [ (e_i - mean(e)) / sd  -  z_i d sd / sd ],      d sd = sum_j (x_j - mean) e_j / ((D - 1) sd)
        |e_i - mean(e)| <= 2 eps;   |d sd| <= eps sum_j |x_j - mean| / ((D - 1) sd) <= eps sqrt(D / (D - 1))     (Cauchy-Schwarz)
        |d out_i| <= |w_i| (eps / sd) (2 + sqrt(D / (D - 1)) |z_i|)
    The leg's own tolerance tol (LayerNorm arithmetic on an exact input) is added: bound = tol + max_i |d out_i| / max |out_ref|.
    (Second order is (eps / sd)^2: below 1e-8 wherever these suites use it.)"""
    x_ref = np.asarray(x_ref, np.float64); D = x_ref.size
    mean = x_ref.mean(); sd = np.sqrt(((x_ref - mean) ** 2).sum() / (D - 1.0))
    z = (x_ref - mean) / sd
    d_out = np.abs(w) * (eps / sd) * (2.0 + np.sqrt(D / (D - 1.0)) * np.abs(z))
    return tol + float(d_out.max()) / max(float(np.abs(out_ref).max()), 1e-30)


# ---- the plain f64 evaluation -------------------------------------------------------------------------------------------------
def _deq(t, wslot, rslot, oslot, layer, N, M):
    """u r + o per INPUT row (rwkv.cu:267-295: y[k] += x[j] (w[j][k] r[j] + o[j])), as f64 [N][M]"""
    W = t[wslot].reshape(-1, N, M)[layer].astype(np.float64)
    W *= t[rslot].reshape(-1, N)[layer].astype(np.float64)[:, None]
    W += t[oslot].reshape(-1, N)[layer].astype(np.float64)[:, None]
    return W


def _ln(x, w, b):
    D = x.shape[-1]
    mean = x.mean(axis=-1, keepdims=True)
    sd = np.sqrt(((x - mean) ** 2).sum(axis=-1, keepdims=True) / (D - 1.0))      # unbiased, no epsilon: rwkv.cu:40-57
    return w * ((x - mean) / sd) + b


def f64_stage(t, L, D, l0, l1, rows, state, tokens=None, want_logits=False):
    """Layers [l0, l1) of the GPT-mode forward (rwkv.cu:493-593) over the n rows of one sequence, every product and sum in f64 and no
    intermediate rounded to f32.  rows [n][D] (l0 == 0: taken from the embedding rows of `tokens` through ln0 instead); state: five
    whole [L][D] arrays, updated in place.  Returns dict(x_in, x_mid (behind att_out, last layer of the range), x_out, h (relu(k)^2 of
    that layer), logits or None)."""
    ln = t[mf.LAYERNORMS].reshape(4 * (L + 1), D)
    if l0 == 0:
        rows = _ln(t[mf.EMBED].reshape(mf.VOCAB, D)[np.asarray(tokens, np.int64)].astype(np.float64), ln[0], ln[1])
    x = np.array(rows, np.float64, copy=True)
    x_in = x.copy()
    n = x.shape[0]
    sxy, saa, sbb, spp, sdd = state
    x_mid = h = None
    for l in range(l0, l1):
        lo = slice(l * D, (l + 1) * D)
        c = _ln(x, ln[4 * l + 2], ln[4 * l + 3])
        p = np.vstack([sxy[lo][None, :], c[:-1]])                                  # token shift along the chunk; row 0 takes the state
        sxy[lo] = c[-1]
        kvr = []
        for mix, ws in ((mf.MIXK, (mf.KM, mf.KR, mf.O1)), (mf.MIXV, (mf.VM, mf.VR, mf.O2)), (mf.MIXR, (mf.RM, mf.RR, mf.O3))):
            mk = t[mix][lo]
            kvr.append((mk * c + (1.0 - mk) * p) @ _deq(t, *ws, l, D, D))
        k, v, r = kvr
        u, w = t[mf.BONUS][lo], t[mf.DECAY][lo]
        aa, bb = saa[lo].copy(), sbb[lo].copy()
        y = np.empty_like(x)
        for i in range(n):                                                         # rwkv.cu:242-255
            e1 = np.exp(u + w + k[i])
            y[i] = (1.0 / (1.0 + np.exp(-r[i]))) * ((aa + e1 * v[i]) / (bb + e1))
            ek = np.exp(k[i])
            aa = (aa + ek * v[i]) * np.exp(w)
            bb = (bb + ek) * np.exp(w)
        saa[lo], sbb[lo] = aa, bb
        x_mid = x + y @ _deq(t, mf.ATTOUT, mf.ATTOUTR, mf.ATTOUTO, l, D, D)
        c = _ln(x_mid, ln[4 * l + 4], ln[4 * l + 5])
        p = np.vstack([sdd[lo][None, :], c[:-1]])
        sdd[lo] = c[-1]
        mk, mr = t[mf.FFNMIXK][lo], t[mf.FFNMIXV][lo]
        rr = (mr * c + (1.0 - mr) * p) @ _deq(t, mf.FFNR, mf.FFNRR, mf.FFNRO, l, D, D)
        kk = (mk * c + (1.0 - mk) * p) @ _deq(t, mf.FFNK, mf.FFNKR, mf.FFNKO, l, D, 4 * D)
        h = np.maximum(kk, 0.0) ** 2
        x = x_mid + (h @ _deq(t, mf.FFNV, mf.FFNVR, mf.FFNVO, l, 4 * D, D)) * (1.0 / (1.0 + np.exp(-rr)))
    logits = None
    if want_logits and l1 == L:
        logits = _ln(x, ln[4 * L + 2], ln[4 * L + 3]) @ _deq(t, mf.HEAD, mf.HEADR, mf.HEADO, 0, D, mf.VOCAB)
    return dict(x_in=x_in, x_mid=x_mid, x_out=x, h=h, logits=logits)


# ---- the oracle, row after row --------------------------------------------------------------------------------------------------
def oracle_att_half(oracle, t, x, state, l, L, D, kv=None):
    """the oracle's residual vector behind att_out of layer l (rwkv.cu:535-553) for one row x f64[D]: the pieces oracle_stage_forward
    is made of, in its order.  state: whole [L][D] arrays; xy, aa, bb of layer l advance in place.  kv: a list that receives the row's
    (k, v) as f64.  (tests/test_chunk_cases_cpu.py checks that this IS what oracle_stage_forward computes: ln2 of the last row's result
    is bit-equal to the dd state the stage leaves.)"""
    ln = t[mf.LAYERNORMS].reshape(4 * (L + 1), D)
    ln1 = oracle.layernorm(x[None, :], ln[4 * l + 2: 4 * l + 4])[0]
    kvr_in = oracle.mixatt(ln1, state[0], t[mf.MIXK], t[mf.MIXV], t[mf.MIXR], D, l, L)
    k, v, r = oracle.mm8_three(kvr_in, t[mf.KM], t[mf.VM], t[mf.RM], t[mf.KR], t[mf.VR], t[mf.RR], t[mf.O1], t[mf.O2], t[mf.O3], D, l)
    if kv is not None:
        kv.append((k.astype(np.float64), v.astype(np.float64)))
    y = oracle.wkv_layer(t[mf.DECAY], t[mf.BONUS], k, v, r, state[1], state[2], state[3], D, l, L)
    return oracle.mm8_layer(y, t[mf.ATTOUT], t[mf.ATTOUTR], t[mf.ATTOUTO], D, D, l, y0=x.astype(np.float32)).astype(np.float64)


def oracle_stage_rows(oracle, om, t, L, D, l0, l1, rows, state, tokens=None, want_logits=False):
    """oracle_stage_forward called row after row on `state` (whole [L][D] arrays of slot 0, updated in place) -- the reference of the
    layer tests -- and, beside it on a copy of the state, the att_out half alone, which yields the x_mid the dd bound needs (one-layer
    ranges only), and the aa recurrence of that layer on magnitudes, m <- (m + e^k |v|) e^w from m = |aa| (aa_mag: the sum of the
    absolute values of the terms aa is made of) and from 0 with max |v| of the row in place of |v| (aa_vmax): the scales an element of
    aa can be held to (aa_elem_err).  Returns dict(x_in, x_mid, x_out, logits, aa_mag, aa_vmax)."""
    n = len(tokens) if l0 == 0 else rows.shape[0]
    ln = t[mf.LAYERNORMS].reshape(4 * (L + 1), D)
    if l0 == 0:
        emb = t[mf.EMBED].reshape(mf.VOCAB, D)[np.asarray(tokens, np.int64)].astype(np.float64)
        rows = oracle.layernorm(emb, ln[0:2])
    side = [a.copy() for a in state]
    lo = slice(l0 * D, (l0 + 1) * D)
    aa_mag, aa_vmax, ew = np.abs(state[1][lo]), np.zeros(D), np.exp(t[mf.DECAY][lo].astype(np.float64))
    x_out = np.empty((n, D)); x_mid = np.empty((n, D))
    logits = np.zeros((n, mf.VOCAB), np.float32) if want_logits and l1 == L else None
    for i in range(n):
        x = np.array(rows[i], np.float64, copy=True)
        om.stage_forward(0 if tokens is None else tokens[i], x, l0, l1, state, 0, None if logits is None else logits[i])
        x_out[i] = x
        if l1 - l0 == 1:
            kv = []
            x_mid[i] = oracle_att_half(oracle, t, np.ascontiguousarray(rows[i], np.float64), side, l0, L, D, kv)
            ek, av = np.exp(kv[0][0]), np.abs(kv[0][1])
            aa_mag, aa_vmax = (aa_mag + ek * av) * ew, (aa_vmax + ek * av.max()) * ew
    return dict(x_in=np.asarray(rows, np.float64), x_mid=x_mid, x_out=x_out, logits=logits, aa_mag=aa_mag, aa_vmax=aa_vmax)


def aa_elem_err(got, ref, aa_mag, aa_vmax, tol_v_over_tol):
    """Worst error of state aa ELEMENT BY ELEMENT, as a fraction delta of its own scale -- without the vector's largest element hiding
    the small ones (case f: 40 decades).  aa_i = c_i0 aa0_i + sum_j c_ij v_ij over the chunk's rows j with weights c_ij > 0 made of
    e^k and e^w.  An element cannot be held to its own value (terms of either sign may cancel), but
      * every weight carries a RELATIVE error delta (k is a GEMV output within tol max |k| of the reference, a few 1e-5 absolute, in
        front of exp; this is why the vector-wide aa / bb legs are 1e-4 and not tol): delta sum_j |term_ij| = delta aa_mag_i;
      * every v_ij carries an ABSOLUTE error of tol_v max_i |v_j| (a GEMV output, held to its vector's max like any other):
        tol_v sum_j c_ij max |v_j| = tol_v aa_vmax_i.
    So |d aa_i| <= delta (aa_mag_i + (tol_v / delta) aa_vmax_i); returns the smallest such delta.  tol_v_over_tol = tol_v / delta."""
    return float((np.abs(np.asarray(got, np.float64) - ref) / (aa_mag + tol_v_over_tol * aa_vmax)).max())


def hidden_sq(t, L, D, l, x_mid, dd_prev, ln2_w=None):
    """relu(k)^2 [n][4 D] of layer l's channel mix for the rows x_mid [n][D] behind att_out, in plain f64 (f64_stage's formulae); dd_prev
    [D] is the dd state in front of row 0; ln2_w replaces the layer's ln2 weight row.  What case g's claim is measured on."""
    ln = t[mf.LAYERNORMS].reshape(4 * (L + 1), D)
    lo = slice(l * D, (l + 1) * D)
    c = _ln(np.asarray(x_mid, np.float64), ln[4 * l + 4] if ln2_w is None else ln2_w, ln[4 * l + 5])
    p = np.vstack([dd_prev[None, :], c[:-1]])
    mk = t[mf.FFNMIXK][lo]
    return np.maximum((mk * c + (1.0 - mk) * p) @ _deq(t, mf.FFNK, mf.FFNKR, mf.FFNKO, l, D, 4 * D), 0.0) ** 2


def check_case_g_tail(h, h_plain, what):
    """case g's claim on the hidden vector it produces: relu(k)^2 is heavy-tailed (max >= 20 mean) and the hot ln2 weights are what
    makes it so (max >= 10 x that of the same rows under the plain ln2 weights)"""
    assert h.max() >= 20.0 * h.mean() and h.max() >= 10.0 * h_plain.max(), \
        f"{what}: relu(k)^2 max {h.max():.3g} mean {h.mean():.3g} (plain ln2 weights: max {h_plain.max():.3g})"
