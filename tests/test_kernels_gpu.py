"""Per-kernel parity of the PRODUCTION decode kernels: a token is launched one kernel at a time through
rwkv_debug_launch -- k_first, then k_att / k_attout / k_ffn_rk / k_ffnv of every layer, then k_head: exactly the launches of the
captured token graph, in the form (row registers, 16-row tiles, 4-row tiles) the context runs each class in -- and after every
launch its outputs are read back and compared with the oracle's piece for THAT kernel, evaluated on the kernel's OWN inputs as the
engine holds them (the residual vector and the state it was handed):

   k_att     oracle_layernorm + oracle_mixatt + oracle_mm8_three + oracle_wkv   (rwkv.cu:535-545; kernels :351-392, :58-142, :221-265)
   k_attout  oracle_mm8_one_f64 with the accumulator pre-loaded with f32(x)     (:548-553), state xy
   k_ffn_rk  oracle_layernorm + oracle_mixffn + 2 x oracle_mm8_one_f64, sigmoid, relu^2   (:557-573)
   k_ffnv    oracle_mm8_one_f32 + blockout                                      (:574-577), state dd
   k_head    oracle_layernorm + oracle_mm8_one_f64                              (:585-589)

so the five mm8_one shapes (att_out D->D, ffn_r D->D, ffn_k D->4D, ffn_v 4D->D, head D->V) are checked on the kernels that ship, and a
compensated error inside one launch has a test that names the launch.  k_attout and k_ffnv are ALSO checked against their exact
contract -- the f64 dot product of the vector they were actually handed (YBUF / HBUF and the per-workgroup offset partials) with the
uint8 matrix -- which isolates them from the producer's rounding.  The three LayerNorm-site consumers k_att, k_ffn_rk and k_head have the
analogous leg against a plain f64 evaluation from the engine's own x and state (decode_cases.f64_att / f64_ffn_rk / f64_head) at the same TOL (1e-4
for aa / bb): tests/test_decode_cases_cpu.py holds the oracle to TOL / 2 of f64 on these inputs and the engine's statistics are f64, so no new
number is needed.

The input of those runs is mild -- ln0 of a synthetic embedding row, the baseline state.  The second half of the module plants the residual
vector and the state (tests/decode_cases.py: through the embedding table, ln0 and push_state, so that the site tuple and the B vectors agree with
x): the seven cases of tests/chunk_cases.py, every leg above on two consecutive tokens; cases h and t, where the bound-based fixed-point scale of
the site consumers is 700-1100 x too coarse and within 1e-4 of wrapping, against f64 alone; and a tie of the top logit in both greedy picks."""
import numpy as np
import pytest

from rwkv_cpp_accelerated_amd import modelfile as mf

import chunk_cases as cc
import decode_cases as dcs
from parity import TOL, _close  # noqa: F401  (one number and one reason for it, shared with tests/test_chunk_layers_gpu.py)

pytestmark = pytest.mark.gpu


_T = {}


def _tensors(L, D):
    """the synthetic model of (L, D), built once and kept while consecutive tests use that width (the planted cases change its embedding
    rows for the duration of a test and restore them: decode_cases.planted)"""
    if (L, D) not in _T:
        _T.clear()
        _T[(L, D)] = mf.synthetic_tensors(L, D, seed=4000 + D)
    return _T[(L, D)]


def _check_token(oracle, monkeypatch, D, tile=None, L=2, grid=None, slot=0, token=4242, n_slots=1, plant=None):
    """One token through the production decode kernels, one launch at a time, every launch against its oracle piece (the module's
    docstring).  tile: RWKV_TILE (None = the context's default form); grid: RWKV_GRID (None = one workgroup per CU); the token runs on
    state slot `slot` of `n_slots`, all filled with different random state -- the other slots must come back untouched.  plant: a
    decode_cases.DecodeCase -- its rows are planted behind k_first and run as consecutive tokens on one context, its state is pushed into
    slot 0.  Returns the loaded context's (decode_form, grid, worst error per leg)."""
    import torch
    if tile is None:
        monkeypatch.delenv("RWKV_TILE", raising=False)
    else:
        if tile != "0" and torch.cuda.get_device_properties(0).multi_processor_count != 256:
            pytest.skip("the tile forms are laid out for 256 workgroups")
        monkeypatch.setenv("RWKV_TILE", tile)
    if grid is None:
        monkeypatch.delenv("RWKV_GRID", raising=False)
    else:
        monkeypatch.setenv("RWKV_GRID", str(grid))
    what = f"D={D} L={L} RWKV_TILE={tile} slot={slot}/{n_slots}"
    if plant is None:
        return _run_tokens(oracle, mf.synthetic_tensors(L, D, seed=4000 + D), D, L, slot, n_slots, [token], None, what + f" token={token}")
    assert slot == 0 and n_slots == 1
    c = plant.case
    with dcs.planted(_tensors(L, D), L, D, c.rows, ln2_mul=c.ln2_mul) as t:
        return _run_tokens(oracle, t, D, L, 0, 1, list(dcs.TOKENS[: c.rows.shape[0]]), plant, what + f" case {plant.label}")


def _run_tokens(oracle, t, D, L, slot, n_slots, tokens, plant, what):
    """the body of _check_token: the tokens one after the other on one context of the model t"""
    from rwkv_cpp_accelerated_amd import engine
    V = mf.VOCAB
    m = engine.RWKV(resident=True); m.loadTensors(L, D, t, maxGPT=n_slots)
    G = m.debug_grid()
    LD, so = L * D, slot * L * D                                             # state slot s: elements [s L D, (s + 1) L D) of every array
    st = m.state
    if plant is None:
        # a non-trivial recurrent state (the reference starts from zeros: every mix / WKV term must see real numbers)
        rng = np.random.default_rng(D)
        n = n_slots * LD
        st.statexy[:] = rng.standard_normal(n); st.statedd[:] = rng.standard_normal(n)
        st.stateaa[:] = rng.standard_normal(n); st.statebb[:] = 0.5 + 1.5 * rng.random(n); st.statepp[:] = rng.standard_normal(n)
    else:
        for a, v in zip(st.arrays(), plant.state):
            a[:] = v
    pushed = [a.copy() for a in st.arrays()]
    m.push_state(n_slots)
    if plant is not None:                                                    # the case's claim on the state the context holds, not on what make_case returned
        for a in st.arrays():
            a[:] = 0.0
        m.pull_state(n_slots)
        assert all(np.array_equal(a, p) for a, p in zip(st.arrays(), pushed)), "the state came back other than pushed"
        cc.check_state(plant.case, [a[:D] for a in st.arrays()])
    ln = t[mf.LAYERNORMS].reshape(4 * (L + 1), D)
    worst = {}

    def note(k, e):
        worst[k] = max(worst.get(k, 0.0), e)

    def update(k, got, ref, x_in, msg, tol=TOL):
        """a residual-update leg.  Baseline: tol of the update's max, as ever.  Planted: chunk_cases.update_eps -- tol of the update's max plus
        one f32 ulp at max |x|: the kernel and both references round f32(x) + update to f32 (rwkv.cu:548-553), |x| is no longer ~3, and two
        correct roundings of sums that differ by less than tol may differ by that ulp; noted as a fraction of that bound."""
        if plant is None:
            note(k, _close(got, ref, msg, tol))
            return
        assert np.isfinite(got).all(), msg
        e = dcs.update_err(got, ref, x_in, tol)
        assert e <= 1.0, f"{msg}: {e:.3f} of update_eps = {cc.update_eps(tol, ref, x_in):.3e}"
        note(k + " / update_eps", e)

    gtail = dcs.GTail(_tensors(L, D)[mf.LAYERNORMS].reshape(-1, D)[4]) if plant is not None else None
    for ti, token in enumerate(tokens):
        m.debug_launch(0, 0, token, slot)                                     # k_first: embedding row + ln0 (rwkv.cu:513-524)
        x = m.debug_read("x")
        emb = t[mf.EMBED].reshape(V, D)[token].astype(np.float64)
        note("first x", _close(x, oracle.layernorm(emb[None, :], ln[0:2])[0], "k_first: x = ln0(embedding row)"))
        note("first x (f64)", _close(x, cc._ln(emb, ln[0], ln[1]), "k_first: x vs f64"))
        if plant is not None:
            dcs.check_planted(plant, ti, x)
        for l in range(L):
            lo = slice(l * D, (l + 1) * D)                                   # layer l of one slot's state / of a per-layer vector
            slo = slice(so + l * D, so + (l + 1) * D)                       # ... of the engine's state arrays, slot `slot`
            tag = f"token {ti} layer {l}"
            # ---- k_att: ln1, mixatt, K/V/R, WKV, from the engine's own x and state ----
            m.pull_state(n_slots)
            own = [a[so: so + LD].copy() for a in st.arrays()]              # xy, aa, bb, pp, dd of the token's slot, as the kernel will read them
            oa = dcs.oracle_att(oracle, t, L, D, l, x, own)
            fa = dcs.f64_att(t, L, D, l, x, own)
            y, ln1 = oa["y"], oa["ln1"]
            m.debug_launch(1, l)
            ybuf = m.debug_read("ybuf"); part_a = m.debug_read("part_att"); pmax_a = m.debug_read("pmax_att")
            m.pull_state(n_slots)
            yf = y.astype(np.float32)                                                                  # the att_out GEMV reads it as f32 (rwkv.cu:290)
            note("att y", _close(ybuf, yf * t[mf.ATTOUTR][lo], f"k_att {tag}: gated wkv * att_out scale"))
            note("att aa", _close(st.stateaa[slo], oa["aa"], f"k_att {tag}: state aa", 1e-4))
            note("att bb", _close(st.statebb[slo], oa["bb"], f"k_att {tag}: state bb", 1e-4))
            note("att y (f64)", _close(ybuf, fa["ybuf"], f"k_att {tag}: gated wkv * att_out scale vs f64"))
            note("att aa (f64)", _close(st.stateaa[slo], fa["aa"], f"k_att {tag}: state aa vs f64", 1e-4))
            note("att bb (f64)", _close(st.statebb[slo], fa["bb"], f"k_att {tag}: state bb vs f64", 1e-4))
            if plant is not None and plant.case.name == "f":                  # 40 decades: element by element, as the chunk suite
                e = float(np.abs(st.statebb[slo] / oa["bb"] - 1.0).max())
                assert e <= 1e-4, f"k_att {tag}: state bb, element by element: {e:.3e} > 1e-4"
                note("att bb/elem", e)
                mag, vmax = dcs.aa_scales(t, D, l, own[1][lo], oa["k"], oa["v"])
                e = cc.aa_elem_err(st.stateaa[slo], oa["aa"], mag, vmax, TOL / 1e-4)
                assert e <= 1e-4, f"k_att {tag}: state aa, element by element: {e:.3e} > 1e-4 of its terms' magnitudes (chunk_cases.aa_elem_err)"
                note("att aa/elem", e)
            assert np.array_equal(st.statepp[so: so + LD], own[3]), "pp is carried through (rwkv.cu:257)"
            terms = yf.astype(np.float64) * t[mf.ATTOUTO][lo]
            e_ref = abs(part_a.sum() - terms.sum()) / np.abs(terms).sum()
            if plant is None:
                assert e_ref <= 1e-5, f"k_att {tag}: offset partials"
            else:                                                             # held to the kernel's own YBUF: see k_ffn_rk's partials below
                own_t = ybuf.astype(np.float64) / t[mf.ATTOUTR][lo] * t[mf.ATTOUTO][lo]
                e_own = abs(part_a.sum() - own_t.sum()) / np.abs(own_t).sum()
                assert e_own <= 1e-5, f"k_att {tag}: offset partials vs the kernel's own gated wkv: {e_own:.3e}"
                note("att partials (own y)", e_own)
            note("att partials (oracle y)", e_ref)
            assert abs(float(pmax_a.max()) - float(np.abs(ybuf).max())) <= 1e-12, "per-workgroup maxima of YBUF"
            # ---- k_attout: x = f32(x) + att_out . y, state xy = ln1 ----
            acc0 = x.astype(np.float32)
            x_ref = dcs.oracle_attout(oracle, t, L, D, l, x, y)
            w_att = t[mf.ATTOUT].reshape(L, D, D)[l].astype(np.float64)
            x_contract = (acc0 + (ybuf.astype(np.float64) @ w_att + part_a.sum()).astype(np.float32)).astype(np.float64)
            m.debug_launch(2, l)
            x1 = m.debug_read("x")
            m.pull_state(n_slots)
            update("attout x (oracle)", x1 - x, x_ref - x, x, f"k_attout {tag}: residual update vs oracle_mm8_one")
            update("attout x (contract)", x1 - x, x_contract - x, x, f"k_attout {tag}: residual update vs the f64 product of its own input", 1e-5)
            note("attout xy", _close(st.statexy[slo], ln1, f"k_attout {tag}: state xy = ln1 output"))
            # ---- k_ffn_rk: ln2, mixffn, ffn_r + sigmoid, ffn_k + relu^2, from the engine's own x ----
            of = dcs.oracle_ffn_rk(oracle, t, L, D, l, x1, own)
            ff = dcs.f64_ffn_rk(t, L, D, l, x1, own)
            ln2, sig, h = of["ln2"], of["sig"], of["h"]
            if plant is not None and plant.case.name == "g" and l == 0:       # case g's claim, on the hidden vector THIS launch produces
                gtail.check(t, L, D, x1, own, ff, f"case g {tag}")
            m.debug_launch(3, l)
            rgate = m.debug_read("rgate"); hbuf = m.debug_read("hbuf"); part_f = m.debug_read("part_ffn")
            fvr = t[mf.FFNVR][l * 4 * D: (l + 1) * 4 * D]; fvo = t[mf.FFNVO][l * 4 * D: (l + 1) * 4 * D]
            note("ffn sigmoid(r)", _close(rgate, sig, f"k_ffn_rk {tag}: sigmoid(ffn_r)"))
            note("ffn relu^2(k)", _close(hbuf, h * fvr, f"k_ffn_rk {tag}: relu(ffn_k)^2 * ffn_v scale"))
            note("ffn sigmoid(r) (f64)", _close(rgate, ff["sig"], f"k_ffn_rk {tag}: sigmoid(ffn_r) vs f64"))
            note("ffn relu^2(k) (f64)", _close(hbuf, ff["hbuf"], f"k_ffn_rk {tag}: relu(ffn_k)^2 * ffn_v scale vs f64"))
            terms = h.astype(np.float64) * fvo
            e_ref = abs(part_f.sum() - terms.sum()) / np.abs(terms).sum()
            if plant is None:
                assert e_ref <= 1e-5, f"k_ffn_rk {tag}: offset partials"
            else:
                # On the planted cases the partials are held to the hidden vector the KERNEL produced (HBUF / scale), which is what k_ffnv's contract
                # leg pairs them with.  Against the oracle's h the sum is not a 1e-5 quantity there: the rounding errors d_j of the staged vector
                # reach every row through weights u_jk of mean 127.5, a shift COMMON to the 4 D rows (each within TOL of max h, checked above), which
                # the all-negative offsets add up instead of averaging out: up to 7.7e-6 on the baseline runs, 2.8e-5 on case c at 2048 (noted, not
                # held).  The att_out partials go the same way (case e at 4096 sits at the 1e-5 an unrelated change of the rounding crosses).
                own = hbuf.astype(np.float64) / fvr * fvo
                e_own = abs(part_f.sum() - own.sum()) / np.abs(own).sum()
                assert e_own <= 1e-5, f"k_ffn_rk {tag}: offset partials vs the kernel's own hidden vector: {e_own:.3e}"
                note("ffn partials (own h)", e_own)
            note("ffn partials (oracle h)", e_ref)
            # ---- k_ffnv: x += ffn_v . h * sigmoid(r), state dd = ln2 ----
            x2_ref = dcs.oracle_ffnv(oracle, t, L, D, l, x1, h, sig)                               # blockout (rwkv.cu:407): f32 product
            w_fv = t[mf.FFNV].reshape(L, 4 * D, D)[l].astype(np.float64)
            v_contract = (hbuf.astype(np.float64) @ w_fv + part_f.sum()).astype(np.float32)
            x2_contract = x1 + (v_contract * rgate).astype(np.float64)
            m.debug_launch(4, l)
            x2 = m.debug_read("x")
            m.pull_state(n_slots)
            update("ffnv x (oracle)", x2 - x1, x2_ref - x1, x1, f"k_ffnv {tag}: residual update vs oracle_mm8_one")
            update("ffnv x (contract)", x2 - x1, x2_contract - x1, x1, f"k_ffnv {tag}: residual update vs the f64 product of its own input", 1e-5)
            note("ffnv dd", _close(st.statedd[slo], ln2, f"k_ffnv {tag}: state dd = ln2 output"))
            x = x2
        # ---- k_head: ln_out + head ----
        m.debug_launch(5, 0)
        logits = m.logits(slot + 1)[slot * V: (slot + 1) * V]                                      # (logits row = state slot)
        note("head", _close(logits, dcs.oracle_head(oracle, t, L, D, x), f"k_head token {ti}: logits"))
        note("head (f64)", _close(logits, dcs.f64_head(t, L, D, x), f"k_head token {ti}: logits vs f64"))
    m.pull_state(n_slots)
    for s in range(n_slots):
        if s != slot:
            for name, a, p in zip("xy aa bb pp dd".split(), st.arrays(), pushed):
                assert np.array_equal(a[s * LD: (s + 1) * LD], p[s * LD: (s + 1) * LD]), f"state {name} of slot {s} changed under a token on slot {slot}"
    form = m.decode_form()
    print(f"{what} decode_form={form} grid={G}: worst per leg: "
          + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    m.close()
    return form, G, worst


@pytest.mark.parametrize("D,tile", [(768, None), (2048, None), (2048, "15"), (2560, None), (4096, None), (4096, "0"), (5120, None), (5120, "15")])
def test_each_production_decode_kernel_against_its_oracle_piece(built, oracle, monkeypatch, D, tile):
    _check_token(oracle, monkeypatch, D, tile)


# The loader takes every n_embed that is a multiple of 16 up to 5120.  Off the widths above: workgroup shares of unequal size on 256
# workgroups (3/4 channels at 1008, 4/5 at 1040, 8/9 at 2064, 12/13 at 3088, 15/16 at 4080, 16/17 at 4112, 19/20 at 5104); a last 1 KiB
# step of the quantised vector that is partly filled at every step count S (1008: S = 1; 1040, 2064: S = 2 and 3 with 16 live bytes in
# the last step; 3088, 4080: S = 4; 4112, 5104: S = 5); widths below 256, where most workgroups own no channel; 3072, an even share of
# 12 at S = 3 with a full last step; and the two neighbours of D = 4096, where the tile form must not be chosen.
@pytest.mark.parametrize("D,token", [(3072, 4242), (4080, 4242), (1008, 4242), (1040, 4242), (2064, 4242), (3088, 4242), (4112, 4242),
                                     (5104, mf.VOCAB - 1), (208, 4242), (80, 4242), (48, 4242), (16, 0)])
def test_decode_kernels_over_the_accepted_width_lattice(built, oracle, monkeypatch, D, token):
    form, G, _ = _check_token(oracle, monkeypatch, D, token=token)
    assert form == 0, "the tile forms exist at D = 2048, 4096 and 5120 only"


@pytest.mark.parametrize("D", [2048, 5120])
def test_row_form_decode_kernels_at_the_tile_form_widths(built, oracle, monkeypatch, D):
    """RWKV_TILE=0 where the default is a tile form (masks 13 and 15): the row kernels at S = 2 and at the only S = 5 width that ships."""
    form, _, _ = _check_token(oracle, monkeypatch, D, tile="0")
    assert form == 0


# RWKV_GRID: every grid from ceil(D / 512) to 256 is accepted.  255, 96 and 37 share D out unevenly (768 / 37: 20 and 21 channels, 4096 /
# 255: 16 and 17, ...); 10 is the smallest grid at D = 5120 (exactly 512 channels per workgroup) and at D = 5104 (510 and 511).
@pytest.mark.parametrize("D,grid", [(768, 255), (768, 96), (768, 37), (2560, 255), (2560, 96), (2560, 37), (4096, 255), (4096, 96), (4096, 37),
                                    (5120, 10), (5104, 10)])
def test_decode_kernels_under_a_grid_other_than_one_workgroup_per_cu(built, oracle, monkeypatch, D, grid):
    form, G, _ = _check_token(oracle, monkeypatch, D, grid=grid, L=1 if D > 3000 else 2)
    assert G == grid
    assert form == 0, "the tile forms are laid out for 256 workgroups"


@pytest.mark.parametrize("D", [1040, 4096])
def test_decode_kernels_on_a_state_slot_other_than_0(built, oracle, monkeypatch, D):
    """A context of three state slots, the token on slot 1 (row form with uneven shares at 1040, the default tile form at 4096): slot 1
    follows the oracle, slots 0 and 2 come back bit-equal to what was pushed, the logits land in row 1."""
    _check_token(oracle, monkeypatch, D, slot=1, n_slots=3, token=0 if D == 1040 else mf.VOCAB - 1)


def test_debug_hooks_refuse_what_they_cannot_run_and_round_trip_a_buffer(built):
    """rwkv_debug_launch / _read / _write (include/rwkv_mi355x.h): bad class, foreign layer, bad slot and a wrong-sized write fail with a
    message instead of launching; a vector written into the context comes back unchanged; a context that owns a layer range runs only its own
    layers and, without the head, neither class 5 nor 6."""
    from rwkv_cpp_accelerated_amd import engine, pipeline
    L, D = 3, 768
    t = mf.synthetic_tensors(L, D, seed=77)
    m = engine.RWKV(resident=True); m.loadTensors(L, D, t)
    for bad in (dict(cls=7), dict(cls=-1), dict(cls=2, layer=L), dict(cls=0, slot=5), dict(cls=0, token=mf.VOCAB)):
        with pytest.raises(engine.RWKVError):
            m.debug_launch(bad.get("cls"), bad.get("layer", 0), bad.get("token", 1), bad.get("slot", 0))
    x = np.random.default_rng(1).standard_normal(D)
    m.debug_write("x", x)
    assert np.array_equal(m.debug_read("x"), x)
    with pytest.raises(engine.RWKVError):
        m.debug_write("x", x[: D // 2])
    assert m.debug_grid() >= 1 and m.debug_read("lnstat").shape == (6,)
    m.close()
    st = pipeline.EngineStage(t, L, D, 0, 2, n_slots=1)          # layers [0, 2): no head
    st.m.debug_launch(0, 0, 9, 0)
    for cls in (1, 2, 3, 4):
        st.m.debug_launch(cls, 0)
    st.m.debug_launch(1, 1)
    for cls, layer in ((1, 2), (5, 0), (6, 0)):
        with pytest.raises(engine.RWKVError):
            st.m.debug_launch(cls, layer)
    st.m.close()


# ---- the planted cases of tests/chunk_cases.py on the decode kernels (tests/decode_cases.py) ------------------------------------------
# The parametrisations above all run ln0 of a synthetic embedding row on the baseline state: unit scale, mean near zero.  The accuracy of the
# site consumers depends on the statistics of their input (the fixed-point scale is a BOUND of max |v_m|, kernels.hip.h site_reduce), that of
# k_attout / k_ffnv on the tail of the pre-scaled vector, that of the WKV epilogue on the span of aa / bb.  (width, RWKV_TILE, layers, cases):
# 1040 is the row form with uneven shares and a partly filled last step, 4096 the 16-row tile form, 2048 mask 13, 5120 the 4-row tiles at S = 5.
# Two layers at the narrow widths: layer 1's k_att then consumes a site opened by k_ffnv on the planted residual plus layer 0's updates.
_ALL = ["a", "b-", "b+", "c", "d", "e", "f", "g"]
_PLANTED = [(1040, None, 2, c) for c in _ALL] + [(4096, "15", 1, c) for c in _ALL] + [(2048, "13", 2, c) for c in "cdg"] + [(5120, "15", 1, c) for c in "cdg"]


@pytest.mark.parametrize("D,tile,L,name", _PLANTED)
def test_decode_kernels_on_planted_residual_and_state(built, oracle, monkeypatch, D, tile, L, name):
    """Every leg of _check_token on a planted case: two rows as two consecutive tokens on one context (the second token's token shift sees
    a planted predecessor), case b as one token per magnitude.  Vectors TOL, aa / bb 1e-4 (case f also element by element), the residual
    updates chunk_cases.update_eps, and the f64 legs of the three site consumers."""
    form, _, _ = _check_token(oracle, monkeypatch, D, tile, L=L, plant=dcs.decode_case(name, D, L))
    assert form == (0 if tile is None else int(tile))


@pytest.mark.parametrize("D,tile", [(1040, None), (4096, "15")])
@pytest.mark.parametrize("which", ["h", "t"])
def test_site_scale_bound_loose_and_tight_against_f64(built, monkeypatch, which, D, tile):
    """The two cases beyond the oracle (decode_cases.case_h, case_t), against plain f64 alone and element by element, within the bound
    decode_cases.site_bound derives from the scale rule: h, a common offset of 1e3 (the scale bound is >= 100 x the vector's true maximum: a grid
    that much coarser), on k_att and k_ffn_rk of two consecutive tokens; t, max |C_k|, max |xhat| and max |B_k| on one channel with matching
    signs (the true maximum is >= 0.99 of the bound), on k_att: nothing wrapped -- a wrapped element is 2 amax off, an O(1) error in k."""
    import torch
    from rwkv_cpp_accelerated_amd import engine
    if tile is None:
        monkeypatch.delenv("RWKV_TILE", raising=False)
    else:
        if torch.cuda.get_device_properties(0).multi_processor_count != 256:
            pytest.skip("the tile forms are laid out for 256 workgroups")
        monkeypatch.setenv("RWKV_TILE", tile)
    monkeypatch.delenv("RWKV_GRID", raising=False)
    L = 1
    t0 = _tensors(L, D)
    dc = dcs.case_h(D, L) if which == "h" else dcs.case_t(t0, L, D)
    ratio, vec = {}, {}

    def leg(k, got, ref, bound):
        ratio[k] = max(ratio.get(k, 0.0), dcs.bound_ratio(got, ref, bound))
        vec[k] = max(vec.get(k, 0.0), dcs.rel(got, ref))

    with dcs.planted(t0, L, D, dc.case.rows, ln0_bias=0.0 if which == "t" else None) as t:
        m = engine.RWKV(resident=True); m.loadTensors(L, D, t)
        assert m.decode_form() == (0 if tile is None else int(tile))
        st = m.state
        for a, v in zip(st.arrays(), dc.state):
            a[:] = v
        m.push_state(1)
        for ti, token in enumerate(dcs.TOKENS[: dc.case.rows.shape[0]]):
            m.debug_launch(0, 0, token, 0)
            x = m.debug_read("x")
            m.pull_state(1)
            own = [a.copy() for a in st.arrays()]
            sv = dcs.site_vectors(t, L, D, 0, "att", x, own[0][:D])
            if which == "h":
                assert abs(x.mean()) >= 0.9 * dcs.OFFSET_H and all(s["amax"] >= 100.0 * s["true"] for s in sv), [(s["amax"], s["true"]) for s in sv]
            else:
                j = dc.case.claims["channel"]
                assert j == int(np.argmax(np.abs(sv[0]["C"]))) == int(np.argmax(np.abs(sv[0]["B"]))) == int(np.argmax(np.abs(x - x.mean())))
                assert sv[0]["true"] >= 0.99 * sv[0]["amax"], f"case t: max |v_k| = {sv[0]['true'] / sv[0]['amax']:.6f} of the bound"
            fa = dcs.f64_att(t, L, D, 0, x, own)
            outs = [dcs.site_bound(t, 0, D, s) for s in sv]
            for (exact, _), key in zip(outs, "kvr"):
                assert np.allclose(exact, fa[key], rtol=0.0, atol=1e-9 * np.abs(fa[key]).max()), f"site_vectors is not f64_att's {key}"
            b = dcs.att_bound(t, D, 0, fa, own, *(o[1] for o in outs))
            m.debug_launch(1, 0)
            ybuf = m.debug_read("ybuf")
            m.pull_state(1)
            leg("att y", ybuf, fa["ybuf"], b["ybuf"]); leg("att aa", st.stateaa[:D], fa["aa"], b["aa"]); leg("att bb", st.statebb[:D], fa["bb"], b["bb"])
            if which == "h":
                m.debug_launch(2, 0)
                x1 = m.debug_read("x")
                sf = dcs.site_vectors(t, L, D, 0, "ffn", x1, own[4][:D])
                assert all(s["amax"] >= 100.0 * s["true"] for s in sf), [(s["amax"], s["true"]) for s in sf]
                ff = dcs.f64_ffn_rk(t, L, D, 0, x1, own)
                (ek_, dkk), (er_, drr) = (dcs.site_bound(t, 0, D, s) for s in sf)
                assert np.allclose(ek_, ff["kk"], rtol=0.0, atol=1e-9 * np.abs(ff["kk"]).max()) and np.allclose(er_, ff["rr"], rtol=0.0, atol=1e-9 * np.abs(ff["rr"]).max())
                bf = dcs.ffn_bound(t, D, 0, ff, dkk, drr)
                m.debug_launch(3, 0)
                leg("ffn sigmoid(r)", m.debug_read("rgate"), ff["sig"], bf["sig"]); leg("ffn relu^2(k)", m.debug_read("hbuf"), ff["hbuf"], bf["hbuf"])
                m.debug_launch(4, 0)
        m.close()
    print(f"case {which} D={D} RWKV_TILE={tile}: measured / bound per leg: " + ", ".join(f"{k} {v:.3f}" for k, v in ratio.items())
          + "; max |d| / max |ref| per leg (TOL = 3e-5): " + ", ".join(f"{k} {v:.1e}" for k, v in vec.items()))
    bad = {k: v for k, v in ratio.items() if not v <= 1.0}
    assert not bad, f"case {which} D={D}: outside the derived bound (measured / bound): {bad}"


def test_greedy_picks_break_ties_towards_the_lowest_id_and_never_pick_0(built):
    """k_head + k_argmax_finish (decode_greedy) and k_argmax_rows (+ _finish; decode_batch_greedy) promise "ties -> lowest id, logit 0
    banned".  HEAD's uint8 column of the model's own pick g is copied into other columns: the scales are per INPUT row, so the copies'
    logits are bit-equal to g's (asserted), the largest of the row.  Copies in 0, 1 and V - 1: id 1 is picked -- 0 is banned, 1 < g, and 1, g,
    V - 1 are rows of different workgroups; copies in 0 and V - 1 only: g itself is the lowest."""
    from rwkv_cpp_accelerated_amd import engine
    L, D, V = 1, 256, mf.VOCAB
    t = mf.synthetic_tensors(L, D, seed=606)

    def load(tt):
        m = engine.RWKV(resident=True); m.loadTensors(L, D, tt, maxGPT=2)
        return m

    m = load(t)
    first = g = None
    for cand in (4242, 17, 9001, 123, 31337):
        m.reset_state()
        g = int(m.decode_greedy(cand, 1)[0])
        if 1 < g < V - 1:
            first = cand
            break
    m.close()
    assert first is not None, "no first token whose pick is neither 0, 1 nor V - 1"
    for cols, want in (([0, 1, V - 1], 1), ([0, V - 1], g)):
        head = t[mf.HEAD].reshape(D, V).copy()
        head[:, cols] = head[:, [g]]
        tt = list(t); tt[mf.HEAD] = head.reshape(-1)
        m = load(tt)
        m.reset_state()
        lg = m.forward(first)[:V].copy()
        assert all(lg[c].tobytes() == lg[g].tobytes() for c in cols), f"the copied columns' logits are not bit-equal: {lg[cols]} vs {lg[g]}"
        assert lg[g] == lg[1:].max() and lg[0] == lg.max()
        m.reset_state()
        assert int(m.decode_greedy(first, 1)[0]) == want, f"decode_greedy with the top logit tied in columns {cols + [g]}"
        m.reset_state()
        picks = m.decode_batch_greedy([first, first], 1)
        assert picks.tolist() == [[want], [want]], f"decode_batch_greedy with the top logit tied in columns {cols + [g]}: {picks.tolist()}"
        m.close()
