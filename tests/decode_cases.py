"""The planted cases of tests/chunk_cases.py on the DECODE kernels (tests/test_kernels_gpu.py on the GPU, tests/test_decode_cases_cpu.py
without one): how a residual vector is planted through the tensors a test owns, the oracle's piece and the plain f64 evaluation of every
decode launch, and the two decode-only cases h and t with the bound their outputs are held to.  TEST INFRASTRUCTURE: nothing here is imported
by the product.

PLANTING.  k_att reads its site tuple (sum x, sum x^2, PA, PB, max |x|) and the B vectors from the kernel that produced x, so a vector written
over x would disagree with them.  A row r is planted through the model instead: f32(r) becomes the embedding row of a chosen token, ln0's
weight row becomes sd(r) on every channel (unbiased sd) and its bias row mean(r), so that k_first produces x = sd (r - mean) / sd + mean = r up
to the f32 rounding of the three.  ln0 is one per model: with two tokens it is taken from row 0, and row 1 comes out as an affine image of
itself (scale sd(r0) / sd(r1), shift mean(r0) - mean(r1) ...), which keeps every claim the cases make -- and the claims are checked on the
vector read back behind k_first (chunk_cases.check_rows), not on what make_case returned.  Case b's two magnitudes are therefore two MODELS
of one token each.  The embedding table is changed in place and restored (it is the largest tensor); the LayerNorm rows are a copy.

REDUCED CONSTANTS.  None: every case of chunk_cases.py held the cap of tests/test_decode_cases_cpu.py (the oracle's pieces within half of
each GPU leg's bound of f64) at n = 2 through ln0 with the constants of the chunk suite; the measured values are in that module's docstring.

h AND t are beyond the oracle (the reference itself is 1e-4 from f64 at an offset of 1e3, chunk_cases.py) and are held to f64 alone, by a
bound DERIVED from the kernels' contract (kernels.hip.h site_reduce / stage_quad / row_value), restated in site_bound."""
from __future__ import annotations

import contextlib
from dataclasses import dataclass

import numpy as np

from rwkv_cpp_accelerated_amd import modelfile as mf

import chunk_cases as cc

TOKENS = (4242, 17)                     # the ids whose embedding rows carry the planted rows
OFFSET_H = 1e3
QLIM = 4194000.0                        # kernels.hip.h: |quantised activation| <= QLIM < 2^22
FLT_MIN = 2.0 ** -126                   # the smallest normal f32


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def _lnrows(t, L, D):
    return t[mf.LAYERNORMS].reshape(4 * (L + 1), D)


@contextlib.contextmanager
def planted(t, L, D, rows, tokens=TOKENS, ln2_mul=None, ln0_bias=None):
    """the model `t` with rows [n][D] planted behind k_first for the n ids `tokens` (the module's docstring) and ln2 of layer 0 multiplied by
    ln2_mul (case g): yields a NEW tensor list that shares every tensor with t but the LayerNorm rows; t's embedding rows are changed for
    the duration of the block and restored behind it.  ln0_bias: replaces mean(rows[0]) (case t wants exactly 0)."""
    rows = np.asarray(rows, np.float64)
    emb = t[mf.EMBED].reshape(mf.VOCAB, D)
    ids = [int(k) for k in tokens[: rows.shape[0]]]
    saved = emb[ids].copy()
    tt = list(t)
    ln = _lnrows(t, L, D).copy()
    ln[0] = _f32(np.full(D, rows[0].std(ddof=1)))
    ln[1] = _f32(np.full(D, rows[0].mean() if ln0_bias is None else ln0_bias))
    if ln2_mul is not None:
        ln[4] = _f32(ln[4] * ln2_mul)
    tt[mf.LAYERNORMS] = ln.reshape(-1)
    try:
        emb[ids] = rows.astype(np.float32)
        yield tt
    finally:
        emb[ids] = saved


@dataclass
class DecodeCase:
    """one planted decode run: `case` (a chunk_cases.Case whose rows are the tokens of the run, in order), its label, the five whole [L][D]
    state arrays to push into slot 0 (the case's vectors in layer 0, the baseline elsewhere)"""
    label: str
    case: cc.Case
    state: list


def decode_case(name, D, L, seed=23):
    """name: a letter of chunk_cases.CASES, or 'b-' / 'b+' -- the row of case b at 10^(TOP_B - 6) / at 10^TOP_B, one token each"""
    c = cc.make_case(name[0], D, 2, seed)
    cc.check_case(c)
    if name[0] == "b":
        rms = np.sqrt((c.rows ** 2).mean(axis=1))
        i = int(np.argmin(rms) if name == "b-" else np.argmax(rms))
        want = 10.0 ** (cc.TOP_B - 6.0 if name == "b-" else cc.TOP_B)
        assert name in ("b-", "b+") and 0.9 * want <= rms[i] <= 1.1 * want, (name, rms)
        c = cc.Case("b", c.rows[i: i + 1].copy(), c.state, c.ln2_mul, dict(c.claims, row_rms=float(rms[i])))
    return DecodeCase(name, c, cc.embed_state(c.state, L, D, 0, seed))


def check_planted(dc: DecodeCase, i, x):
    """the case's claim on row i AS READ BACK behind k_first (x [D]): a case must not be able to degenerate on its way through the embedding
    table and ln0.  Row 0 is the row ln0 was made from and comes back as itself; case b's claim is its magnitude."""
    c = dc.case
    if i == 0:
        d = float(np.abs(x - c.rows[0]).max()) / float(np.abs(c.rows[0]).max())
        assert d <= 1e-5, f"case {dc.label}: the planted row came back {d:.1e} of its max from itself"
    if c.name == "b":
        rms = float(np.sqrt((x ** 2).mean()))
        assert abs(rms / c.claims["row_rms"] - 1.0) <= 1e-3, f"case {dc.label}: rms {rms:.3e} behind k_first, planted {c.claims['row_rms']:.3e}"
    cc.check_rows(c, x[None, :])


# ---- a launch's reference, twice: the oracle's piece (what the reference computes, its f32 roundings included) and plain f64 -------------
def matvec64(a, t, wslot, rslot, oslot, layer, N, M):
    """a f64[N] times layer `layer` of a stacked uint8 matrix, dequantised as chunk_cases._deq does (u r + o per INPUT row, f64), in blocks
    of input rows so that the f64 image of a D x 4 D or D x VOCAB matrix never exists as a whole"""
    W8 = t[wslot].reshape(-1, N, M)[layer]
    r = t[rslot].reshape(-1, N)[layer].astype(np.float64); o = t[oslot].reshape(-1, N)[layer].astype(np.float64)
    out = np.zeros(M)
    step = max(16, (1 << 24) // M)
    for j in range(0, N, step):
        W = W8[j: j + step].astype(np.float64)
        W *= r[j: j + step, None]
        W += o[j: j + step, None]
        out += a[j: j + step] @ W
    return out


def oracle_att(oracle, t, L, D, l, x, state):
    """k_att's oracle piece (rwkv.cu:535-545) on the residual vector x and one slot's state (five [L][D] arrays, not changed): dict(ln1, y
    (the gated wkv, f64), aa, bb (layer l's new state, [D]))"""
    ln = _lnrows(t, L, D)
    lo = slice(l * D, (l + 1) * D)
    ln1 = oracle.layernorm(x[None, :], ln[4 * l + 2: 4 * l + 4])[0]
    sxy = state[0].copy()
    kvr_in = oracle.mixatt(ln1, sxy, t[mf.MIXK], t[mf.MIXV], t[mf.MIXR], D, l, L)                  # (writes ln1 into sxy[l])
    k, v, r = oracle.mm8_three(kvr_in, t[mf.KM], t[mf.VM], t[mf.RM], t[mf.KR], t[mf.VR], t[mf.RR], t[mf.O1], t[mf.O2], t[mf.O3], D, l)
    aa, bb, pp = state[1].copy(), state[2].copy(), state[3].copy()
    y = oracle.wkv_layer(t[mf.DECAY], t[mf.BONUS], k, v, r, aa, bb, pp, D, l, L)
    return dict(ln1=ln1, y=y, aa=aa[lo], bb=bb[lo], k=k.astype(np.float64), v=v.astype(np.float64))


def oracle_ffn_rk(oracle, t, L, D, l, x1, state):
    """k_ffn_rk's oracle piece (rwkv.cu:557-573) on the residual vector behind att_out: dict(ln2, sig (sigmoid(ffn_r), f32), h (relu(ffn_k)^2, f32))"""
    ln = _lnrows(t, L, D)
    ln2 = oracle.layernorm(x1[None, :], ln[4 * l + 4: 4 * l + 6])[0]
    sdd = state[4].copy()
    k_in, r_in = oracle.mixffn(ln2, sdd, t[mf.FFNMIXK], t[mf.FFNMIXV], D, l, L)
    rr = oracle.mm8_layer(r_in, t[mf.FFNR], t[mf.FFNRR], t[mf.FFNRO], D, D, l)
    sig = (1.0 / (1.0 + np.exp(-rr.astype(np.float64)))).astype(np.float32)                        # rwkv.cu:212
    kk = oracle.mm8_layer(k_in, t[mf.FFNK], t[mf.FFNKR], t[mf.FFNKO], D, 4 * D, l)
    h = kk * (kk > 0).astype(np.float32); h = h * h                                                # rwkv.cu:189-190
    return dict(ln2=ln2, sig=sig, h=h)


def oracle_attout(oracle, t, L, D, l, x, y):
    """k_attout's oracle piece (rwkv.cu:548-553): the accumulator pre-loaded with f32(x), plus att_out . y; f64[D]"""
    return oracle.mm8_layer(y, t[mf.ATTOUT], t[mf.ATTOUTR], t[mf.ATTOUTO], D, D, l, y0=x.astype(np.float32)).astype(np.float64)


def oracle_ffnv(oracle, t, L, D, l, x1, h, sig):
    """k_ffnv's oracle piece (rwkv.cu:574-577): x1 + f32(ffn_v . h) * sigmoid(r), the product in f32 (blockout, :407)"""
    vv = oracle.mm8_layer(h, t[mf.FFNV], t[mf.FFNVR], t[mf.FFNVO], 4 * D, D, l)
    return x1 + (vv * sig).astype(np.float64)


def oracle_head(oracle, t, L, D, x):
    """k_head's oracle piece (rwkv.cu:585-589)"""
    ln = _lnrows(t, L, D)
    lno = oracle.layernorm(x[None, :], ln[4 * L + 2: 4 * L + 4])[0]
    return oracle.mm8_layer(lno, t[mf.HEAD], t[mf.HEADR], t[mf.HEADO], D, mf.VOCAB, 0)


def f64_att(t, L, D, l, x, state):
    """what k_att computes, in plain f64 (chunk_cases.f64_stage's formulae for one row) from the residual vector x and one slot's state as
    the ENGINE holds them: dict(ybuf (gated wkv times the att_out scale), aa, bb, and k, v, r, wkv for the bounds of cases h and t)"""
    ln = _lnrows(t, L, D)
    lo = slice(l * D, (l + 1) * D)
    c = cc._ln(np.asarray(x, np.float64), ln[4 * l + 2], ln[4 * l + 3])
    p = state[0][lo]
    kvr = []
    for mix, ws in ((mf.MIXK, (mf.KM, mf.KR, mf.O1)), (mf.MIXV, (mf.VM, mf.VR, mf.O2)), (mf.MIXR, (mf.RM, mf.RR, mf.O3))):
        mk = t[mix][lo]
        kvr.append(matvec64(mk * c + (1.0 - mk) * p, t, *ws, l, D, D))
    k, v, r = kvr
    u, w = t[mf.BONUS][lo], t[mf.DECAY][lo]
    aa, bb = state[1][lo], state[2][lo]
    e1, ek = np.exp(u + w + k), np.exp(k)
    wkv = (aa + e1 * v) / (bb + e1)
    y = wkv / (1.0 + np.exp(-r))
    return dict(ybuf=y * t[mf.ATTOUTR][lo], aa=(aa + ek * v) * np.exp(w), bb=(bb + ek) * np.exp(w), k=k, v=v, r=r, wkv=wkv, e1=e1, ek=ek)


def f64_ffn_rk(t, L, D, l, x1, state, ln2_w=None, prev=None):
    """what k_ffn_rk computes, in plain f64: dict(sig, hbuf (relu(ffn_k)^2 times the ffn_v scale), h, kk, rr, ln2); ln2_w replaces the layer's
    ln2 weight row and prev the dd state in front of the token (case g's claim is measured against the same rows under the plain weights,
    whose token shift has to see the predecessor under the plain weights too)"""
    ln = _lnrows(t, L, D)
    lo = slice(l * D, (l + 1) * D)
    c = cc._ln(np.asarray(x1, np.float64), ln[4 * l + 4] if ln2_w is None else ln2_w, ln[4 * l + 5])
    p = state[4][lo] if prev is None else prev
    mk, mr = t[mf.FFNMIXK][lo], t[mf.FFNMIXV][lo]
    rr = matvec64(mr * c + (1.0 - mr) * p, t, mf.FFNR, mf.FFNRR, mf.FFNRO, l, D, D)
    kk = matvec64(mk * c + (1.0 - mk) * p, t, mf.FFNK, mf.FFNKR, mf.FFNKO, l, D, 4 * D)
    h = np.maximum(kk, 0.0) ** 2
    return dict(sig=1.0 / (1.0 + np.exp(-rr)), hbuf=h * t[mf.FFNVR][l * 4 * D: (l + 1) * 4 * D], h=h, kk=kk, rr=rr, ln2=c)


def f64_head(t, L, D, x):
    """what k_head computes, in plain f64"""
    ln = _lnrows(t, L, D)
    return matvec64(cc._ln(np.asarray(x, np.float64), ln[4 * L + 2], ln[4 * L + 3]), t, mf.HEAD, mf.HEADR, mf.HEADO, 0, D, mf.VOCAB)


class GTail:
    """case g's claim (chunk_cases.check_case_g_tail) on the hidden vector of every token of a run: relu(k)^2 under the hot ln2 weights of
    layer 0 against the same residual vectors under the model's plain ln2 weights, token after token"""

    def __init__(self, plain_ln2_w):
        self.w, self.prev = plain_ln2_w, None

    def check(self, t, L, D, x1, state, ff, what):
        plain = f64_ffn_rk(t, L, D, 0, x1, state, ln2_w=self.w, prev=self.prev)
        self.prev = plain["ln2"]
        cc.check_case_g_tail(ff["h"], plain["h"], what)


def rel(got, ref):
    """max |got - ref| / max |ref|: the figure parity._close holds to a tolerance"""
    return float(np.abs(np.asarray(got, np.float64) - ref).max()) / max(float(np.abs(ref).max()), 1e-30)


def update_err(got_upd, ref_upd, x_in, tol):
    """the error of a residual update as a multiple of chunk_cases.update_eps(tol, ...): <= 1 is inside"""
    return float(np.abs(np.asarray(got_upd, np.float64) - ref_upd).max()) / cc.update_eps(tol, ref_upd, x_in)


# ---- cases h and t ----------------------------------------------------------------------------------------------------------------------
def site_vectors(t, L, D, l, site, x, prev):
    """The LayerNorm-site contract of DESIGN.md 4.2, restated: for the vectors m of `site` ('att': K, V, R behind ln1; 'ffn': ffn_k, ffn_r
    behind ln2) the consumer stages v_m[j] = C_m[j] xhat[j] + B_m[j] with C_m = r_m mix_m lnw, B_m = r_m (mix_m lnb + (1 - mix_m) prev[j]),
    xhat = (x - mean) rstd, quantised on a grid of amax_m / QLIM where amax_m is NOT the measured maximum but the bound
        amax_m = 1.0001 (maxC_m (max |x| + |mean|) rstd + max |B_m|)                                  (kernels.hip.h site_reduce).
    Returns a list of dict(v, C, B, amax, true (= max |v_m|), w (wslot, rslot, oslot), M) in plain f64."""
    ln = _lnrows(t, L, D)
    lo = slice(l * D, (l + 1) * D)
    x = np.asarray(x, np.float64)
    if site == "att":
        lnw, lnb = ln[4 * l + 2], ln[4 * l + 3]
        vecs = [(mf.MIXK, (mf.KM, mf.KR, mf.O1), D), (mf.MIXV, (mf.VM, mf.VR, mf.O2), D), (mf.MIXR, (mf.RM, mf.RR, mf.O3), D)]
    else:
        lnw, lnb = ln[4 * l + 4], ln[4 * l + 5]
        vecs = [(mf.FFNMIXK, (mf.FFNK, mf.FFNKR, mf.FFNKO), 4 * D), (mf.FFNMIXV, (mf.FFNR, mf.FFNRR, mf.FFNRO), D)]
    mean = x.mean(); rstd = 1.0 / np.sqrt(((x - mean) ** 2).sum() / (D - 1.0))
    xhat = (x - mean) * rstd
    out = []
    for mix, w, M in vecs:
        r = t[w[1]].reshape(-1, D)[l].astype(np.float64)
        mk = t[mix][lo]
        C = r * mk * lnw
        B = r * (mk * lnb + (1.0 - mk) * prev)
        v = C * xhat + B
        amax = 1.0001 * (np.abs(C).max() * (np.abs(x).max() + abs(mean)) * rstd + np.abs(B).max())
        out.append(dict(v=v, C=C, B=B, amax=float(amax), true=float(np.abs(v).max()), w=w, M=M))
    return out


def site_bound(t, l, D, sv):
    """Per-element bound of a site consumer's GEMV output out_k = sum_j v_j u_jk + S, S = sum_j x'_j o_j, against its exact value, DERIVED
    from the contract (nothing here is measured):
      * v_j is formed in f32 from an f64 subtraction -- one cast, one multiply, one fma, each within 2^-24 of a value <= amax -- and
        rounded to the grid step = amax / QLIM: |d v_j| <= step / 2 + 2^-22 amax.  (With the bound as scale nothing WRAPS: |v| / step <= QLIM
        < 2^22.  A vector past the bound would leave its three limbs and come back 2^23 steps = 2 amax off: an O(1) error.)
      * the integer sums are exact, so |d out_k| <= (step / 2 + 2^-22 amax) sum_j u_jk
      * the finish rounds the f64 row value and the offset scalar to f32 and adds them in f32 (row_value + S):
        2^-23 (|sum_j v_j u_jk| + |S|) covers the three roundings.
    Returns (exact out f64[M], bound f64[M])."""
    ws, rs, os_ = sv["w"]
    M = sv["M"]
    U = t[ws].reshape(-1, D, M)[l]
    r = t[rs].reshape(-1, D)[l].astype(np.float64); o = t[os_].reshape(-1, D)[l].astype(np.float64)
    main = np.zeros(M); colsum = np.zeros(M)
    step_rows = max(16, (1 << 24) // M)
    for j in range(0, D, step_rows):
        W = U[j: j + step_rows].astype(np.float64)
        main += sv["v"][j: j + step_rows] @ W
        colsum += W.sum(axis=0)
    S = float((sv["v"] / r) @ o)
    dv = (0.5 / QLIM + 2.0 ** -22) * sv["amax"] * (1.0 + 2.0 ** -20)         # (the kernel's amax is this one formed in f32)
    return main + S, dv * colsum + 2.0 ** -23 * (np.abs(main) + abs(S))


def case_h(D, L, seed=29):
    """h, the LOOSE bound: a common offset of OFFSET_H on unit-variance rows.  max |x| + |mean| is ~2000 where max |x - mean| is ~4: the
    scale bound, and with it the quantisation grid, is some 500 x coarser than the vector needs.  Two rows (two tokens)."""
    rng = np.random.default_rng([seed, D, 7])
    rows = rng.standard_normal((2, D)) + OFFSET_H
    c = cc.Case("h", rows, cc.baseline_state(rng, D), np.ones(D), {})
    return DecodeCase("h", c, cc.embed_state(c.state, L, D, 0, seed))


def case_t(t, L, D, seed=31):
    """t, the TIGHT bound, for the k vector of layer 0's ln1 site in the model t: ONE outlier on the channel j* of the largest |C_k|, large
    enough to be max |xhat| whatever the rest does, the state xy (prev) on j* large enough that |B_k[j*]| is max |B_k|, both with signs that make
    C xhat and B add up, and the row balanced to mean 0 (ln0's bias is planted as exactly 0).  Then max |v_k| is the bound up to its two guard
    factors (1.0000002 on max |x|, 1.0001 on the sum).  One row."""
    rng = np.random.default_rng([seed, D, 8])
    ln = _lnrows(t, L, D)
    mk = t[mf.MIXK][:D]
    r = t[mf.KR].reshape(-1, D)[0].astype(np.float64)
    C = r * mk * ln[2]
    j = int(np.argmax(np.abs(C)))
    state = cc.baseline_state(rng, D)
    row = rng.standard_normal(D)
    row[j] = 0.0
    row -= row.sum() / (D - 1.0)                                            # the others sum to zero ...
    row[j] = 0.0
    A = -40.0 * np.sign(C[j])                                                # ... and stay so: A on j*, -A / (D - 1) on each of the others.  C xhat < 0:
    # the NEGATIVE end of the grid is the one that matters -- stage_quad's float 1.5 2^23 + q drops a binade below q = -2^22 and the element comes
    # back 2^23 steps off, where above +2^22 it only loses a bit (half the excess)
    row[j] = A
    row[np.arange(D) != j] -= A / (D - 1.0)
    sgn = np.sign(C[j] * A)                                                  # sign of C xhat on j*: B has to agree
    state[0][j] = sgn * 60.0 / (1.0 - mk[j])                                 # (1 - mix) prev = 60 >> |mix lnb| and any other channel's 4-sigma prev
    c = cc.Case("t", row[None, :], state, np.ones(D), dict(channel=j))
    return DecodeCase("t", c, cc.embed_state(c.state, L, D, 0, seed))


def aa_scales(t, D, l, aa0, k, v):
    """the two scales chunk_cases.aa_elem_err holds an element of the new aa to, for ONE token on the state aa0 [D] (oracle_stage_rows'
    recurrence, one step): aa_mag = (|aa0| + e^k |v|) e^w, aa_vmax = e^k max |v| e^w"""
    ew = np.exp(t[mf.DECAY][l * D: (l + 1) * D].astype(np.float64))
    ek, av = np.exp(k), np.abs(v)
    return (np.abs(aa0) + ek * av) * ew, ek * av.max() * ew


def att_bound(t, D, l, fa, state, dk, dv, dr):
    """Per-element bounds of k_att's three outputs from per-element bounds dk, dv, dr of its K / V / R rows (site_bound), through the WKV
    epilogue (rwkv.cu:242-255; fa = f64_att's result on the same x and state; bb > 0):
       y = sigmoid(r) wkv,  wkv = (aa + e1 v) / (bb + e1),  e1 = e^(u + w + k);    aa' = (aa + e^k v) e^w;    bb' = (bb + e^k) e^w.
    Each is MONOTONE in each of k, v, r with the others held (d wkv / dk = e1 (v bb - aa) / (bb + e1)^2 has the sign of v bb - aa whatever k is,
    wkv and aa' are linear in v, sigmoid is monotone and multiplies a wkv of fixed sign), so over the box [k +- dk] x [v +- dv] x [r +- dr] the
    extremes are at its corners: the bound is the largest deviation over the 8 corners -- no linearisation, dk need not be small.  On top, the
    f32 steps behind the rows: expf(-r) and the gate (a relative 2^-22 on y), the cast of y and its product with the att_out scale (2^-24 each):
    2^-21 |ybuf| covers them, and ybuf is an f32: below FLT_MIN = 2^-126 a gate or a product may flush to zero (case t has r down to -170, a gate
    of 1e-75), which is an ABSOLUTE FLT_MIN (1 + |wkv scale|).  The state is f64 arithmetic on the f32 k and v: 2^-40."""
    lo = slice(l * D, (l + 1) * D)
    aa0, bb0 = state[1][lo], state[2][lo]
    assert (bb0 > 0).all()
    u, w = t[mf.BONUS][lo], t[mf.DECAY][lo]
    ra = np.abs(t[mf.ATTOUTR][lo].astype(np.float64))
    by = np.zeros(D); ba = np.zeros(D); bb = np.zeros(D)
    for sk in (-1.0, 1.0):
        k = fa["k"] + sk * dk
        e1, ek = np.exp(u + w + k), np.exp(k)
        bb = np.maximum(bb, np.abs((bb0 + ek) * np.exp(w) - fa["bb"]))
        for sv in (-1.0, 1.0):
            v = fa["v"] + sv * dv
            ba = np.maximum(ba, np.abs((aa0 + ek * v) * np.exp(w) - fa["aa"]))
            wkv = (aa0 + e1 * v) / (bb0 + e1)
            for sr in (-1.0, 1.0):
                by = np.maximum(by, np.abs(wkv / (1.0 + np.exp(-(fa["r"] + sr * dr))) * ra - fa["ybuf"]))
    tiny = FLT_MIN * (1.0 + np.abs(fa["wkv"]) * ra)                          # expf(-r) overflows for r < -88.7: the gate, below FLT_MIN, comes out 0
    return dict(ybuf=by + 2.0 ** -21 * np.abs(fa["ybuf"]) + tiny, aa=ba + 2.0 ** -40 * np.abs(fa["aa"]), bb=bb + 2.0 ** -40 * np.abs(fa["bb"]))


def ffn_bound(t, D, l, ff, dkk, drr):
    """Per-element bounds of k_ffn_rk's two outputs from those of its ffn_k / ffn_r rows; both are monotone in their row, so the extremes are at
    k +- dk, r +- dr: sigmoid (plus 2^-22 for expf and the f32 divide of a value <= 1) and relu(k)^2 times the ffn_v scale (plus 2^-22 |hbuf| for
    the two f32 products and FLT_MIN: hbuf is an f32, and where k + dk < 0 it is exactly 0 on both sides)"""
    fvr = t[mf.FFNVR][l * 4 * D: (l + 1) * 4 * D].astype(np.float64)
    sig = np.maximum(np.abs(1.0 / (1.0 + np.exp(-(ff["rr"] + drr))) - ff["sig"]), np.abs(1.0 / (1.0 + np.exp(-(ff["rr"] - drr))) - ff["sig"]))
    h = np.maximum(np.abs(np.maximum(ff["kk"] + dkk, 0.0) ** 2 - ff["h"]), np.abs(np.maximum(ff["kk"] - dkk, 0.0) ** 2 - ff["h"]))
    return dict(sig=sig + 2.0 ** -22, hbuf=h * fvr + 2.0 ** -22 * np.abs(ff["hbuf"]) + FLT_MIN)


def bound_ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound: <= 1 is inside.  An element that is exact is inside whatever its bound; NaN never is."""
    d = np.abs(np.asarray(got, np.float64) - ref)
    assert np.isfinite(d).all() and np.isfinite(bound).all() and (bound >= 0).all()
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(d == 0.0, 0.0, d / bound).max())


def emulate_att(t, D, l, x, state, sv, amax_factor=1.0):
    """k_att's arithmetic restated in numpy with its roundings (the f32 C and B tables, xhat and v in f32, the grid of amax / QLIM, exact
    integer sums, the f32 finish of the rows, the f32 expf gate and f32 ybuf): what tests/test_decode_cases_cpu.py holds the derived bounds
    to without a GPU.  amax_factor scales the bound-based scale (a factor below 1 on case t takes the largest element past -2^22, where the
    float leaves its binade and the three bytes are no longer the limbs: it comes back 2^23 steps off).  Returns dict(ybuf, aa, bb, qmax)."""
    f32 = np.float32
    lo = slice(l * D, (l + 1) * D)
    x = np.asarray(x, np.float64)
    mean = x.mean(); rstd = 1.0 / np.sqrt(((x - mean) ** 2).sum() / (D - 1.0))
    rows, qmax = [], 0.0
    for s in sv:
        amax = f32(s["amax"] * amax_factor)
        xh = (x - mean).astype(f32) * f32(rstd)
        v = (s["C"].astype(f32).astype(np.float64) * xh + s["B"].astype(f32).astype(np.float64)).astype(f32)
        f = (v.astype(np.float64) * np.float64(f32(QLIM) / amax) + 1.5 * 2.0 ** 23).astype(f32)     # stage_quad: one fma scales, rounds and offsets
        qmax = max(qmax, float(np.abs(f.astype(np.float64) - 1.5 * 2.0 ** 23).max()))
        q = (f.view(np.uint32) & np.uint32(0xFFFFFF)).astype(np.float64) - 2.0 ** 22                    # its low three bytes ARE the limbs of q + 2^22
        U = t[s["w"][0]].reshape(-1, D, s["M"])[l].astype(np.float64)
        r_ = t[s["w"][1]].reshape(-1, D)[l].astype(np.float64); o_ = t[s["w"][2]].reshape(-1, D)[l].astype(np.float64)
        rows.append(((q @ U) * (np.float64(amax) / QLIM)).astype(f32) + f32((s["v"] / r_) @ o_))
    k, v, r = rows[0].astype(np.float64), rows[1].astype(np.float64), rows[2]
    u, w = t[mf.BONUS][lo], t[mf.DECAY][lo]
    aa0, bb0 = state[1][lo], state[2][lo]
    e1, ek = np.exp(u + w + k), np.exp(k)
    with np.errstate(over="ignore"):
        y = (1.0 / (1.0 + np.exp(-r).astype(np.float64))) * ((aa0 + e1 * v) / (bb0 + e1))
    return dict(ybuf=y.astype(f32) * t[mf.ATTOUTR][lo].astype(f32), aa=(aa0 + ek * v) * np.exp(w), bb=(bb0 + ek) * np.exp(w), qmax=qmax)
