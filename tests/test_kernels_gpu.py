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
uint8 matrix -- which isolates them from the producer's rounding."""
import numpy as np
import pytest

from rwkv_cpp_accelerated_amd import modelfile as mf

from parity import TOL, _close  # noqa: F401  (one number and one reason for it, shared with tests/test_chunk_layers_gpu.py)

pytestmark = pytest.mark.gpu


def _check_token(oracle, monkeypatch, D, tile=None, L=2, grid=None, slot=0, token=4242, n_slots=1):
    """One token through the production decode kernels, one launch at a time, every launch against its oracle piece (the module's
    docstring).  tile: RWKV_TILE (None = the context's default form); grid: RWKV_GRID (None = one workgroup per CU); the token runs on
    state slot `slot` of `n_slots`, all filled with different random state -- the other slots must come back untouched.  Returns the
    loaded context's (decode_form, grid, worst error per leg)."""
    import torch
    from rwkv_cpp_accelerated_amd import engine
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
    V = mf.VOCAB
    t = mf.synthetic_tensors(L, D, seed=4000 + D)
    m = engine.RWKV(resident=True); m.loadTensors(L, D, t, maxGPT=n_slots)
    G = m.debug_grid()
    LD, so = L * D, slot * L * D                                             # state slot s: elements [s L D, (s + 1) L D) of every array
    # a non-trivial recurrent state (the reference starts from zeros: every mix / WKV term must see real numbers)
    rng = np.random.default_rng(D)
    st = m.state
    n = n_slots * LD
    st.statexy[:] = rng.standard_normal(n); st.statedd[:] = rng.standard_normal(n)
    st.stateaa[:] = rng.standard_normal(n); st.statebb[:] = 0.5 + 1.5 * rng.random(n); st.statepp[:] = rng.standard_normal(n)
    pushed = [a.copy() for a in st.arrays()]
    m.push_state(n_slots)
    ln = t[mf.LAYERNORMS].reshape(4 * (L + 1), D)
    worst = {}

    def note(k, e):
        worst[k] = max(worst.get(k, 0.0), e)

    m.debug_launch(0, 0, token, slot)                                         # k_first: embedding row + ln0 (rwkv.cu:513-524)
    x = m.debug_read("x")
    emb = t[mf.EMBED].reshape(V, D)[token].astype(np.float64)
    note("first x", _close(x, oracle.layernorm(emb[None, :], ln[0:2])[0], "k_first: x = ln0(embedding row)"))
    for l in range(L):
        lo = slice(l * D, (l + 1) * D)                                       # layer l of one slot's state / of a per-layer vector
        slo = slice(so + l * D, so + (l + 1) * D)                           # ... of the engine's state arrays, slot `slot`
        # ---- k_att: ln1, mixatt, K/V/R, WKV, from the engine's own x and state ----
        m.pull_state(n_slots)
        sxy, saa, sbb, spp, sdd = (a[so: so + LD].copy() for a in st.arrays())
        ln1 = oracle.layernorm(x[None, :], ln[4 * l + 2: 4 * l + 4])[0]
        sxy_o = sxy.copy()
        kvr_in = oracle.mixatt(ln1, sxy_o, t[mf.MIXK], t[mf.MIXV], t[mf.MIXR], D, l, L)          # (writes ln1 into sxy_o[l])
        k, v, r = oracle.mm8_three(kvr_in, t[mf.KM], t[mf.VM], t[mf.RM], t[mf.KR], t[mf.VR], t[mf.RR], t[mf.O1], t[mf.O2], t[mf.O3], D, l)
        aa_o, bb_o, pp_o = saa.copy(), sbb.copy(), spp.copy()
        y = oracle.wkv_layer(t[mf.DECAY], t[mf.BONUS], k, v, r, aa_o, bb_o, pp_o, D, l, L)
        m.debug_launch(1, l)
        ybuf = m.debug_read("ybuf"); part_a = m.debug_read("part_att"); pmax_a = m.debug_read("pmax_att")
        m.pull_state(n_slots)
        yf = y.astype(np.float32)                                                                  # the att_out GEMV reads it as f32 (rwkv.cu:290)
        note("att y", _close(ybuf, yf * t[mf.ATTOUTR][lo], f"k_att layer {l}: gated wkv * att_out scale"))
        note("att aa", _close(st.stateaa[slo], aa_o[lo], f"k_att layer {l}: state aa", 1e-4))
        note("att bb", _close(st.statebb[slo], bb_o[lo], f"k_att layer {l}: state bb", 1e-4))
        assert np.array_equal(st.statepp[so: so + LD], spp), "pp is carried through (rwkv.cu:257)"
        terms = yf.astype(np.float64) * t[mf.ATTOUTO][lo]
        assert abs(part_a.sum() - terms.sum()) <= 1e-5 * np.abs(terms).sum(), f"k_att layer {l}: offset partials"
        assert abs(float(pmax_a.max()) - float(np.abs(ybuf).max())) <= 1e-12, "per-workgroup maxima of YBUF"
        # ---- k_attout: x = f32(x) + att_out . y, state xy = ln1 ----
        acc0 = x.astype(np.float32)
        x_ref = oracle.mm8_layer(y, t[mf.ATTOUT], t[mf.ATTOUTR], t[mf.ATTOUTO], D, D, l, y0=acc0).astype(np.float64)
        w_att = t[mf.ATTOUT].reshape(L, D, D)[l].astype(np.float64)
        x_contract = (acc0 + (ybuf.astype(np.float64) @ w_att + part_a.sum()).astype(np.float32)).astype(np.float64)
        m.debug_launch(2, l)
        x1 = m.debug_read("x")
        m.pull_state(n_slots)
        note("attout x (oracle)", _close(x1 - x, x_ref - x, f"k_attout layer {l}: residual update vs oracle_mm8_one"))
        note("attout x (contract)", _close(x1 - x, x_contract - x, f"k_attout layer {l}: residual update vs the f64 product of its own input", 1e-5))
        note("attout xy", _close(st.statexy[slo], ln1, f"k_attout layer {l}: state xy = ln1 output"))
        # ---- k_ffn_rk: ln2, mixffn, ffn_r + sigmoid, ffn_k + relu^2, from the engine's own x ----
        ln2 = oracle.layernorm(x1[None, :], ln[4 * l + 4: 4 * l + 6])[0]
        sdd_o = sdd.copy()
        k_in, r_in = oracle.mixffn(ln2, sdd_o, t[mf.FFNMIXK], t[mf.FFNMIXV], D, l, L)
        rr = oracle.mm8_layer(r_in, t[mf.FFNR], t[mf.FFNRR], t[mf.FFNRO], D, D, l)
        sig = (1.0 / (1.0 + np.exp(-rr.astype(np.float64)))).astype(np.float32)                    # rwkv.cu:212
        kk = oracle.mm8_layer(k_in, t[mf.FFNK], t[mf.FFNKR], t[mf.FFNKO], D, 4 * D, l)
        h = kk * (kk > 0).astype(np.float32); h = h * h                                            # rwkv.cu:189-190
        m.debug_launch(3, l)
        rgate = m.debug_read("rgate"); hbuf = m.debug_read("hbuf"); part_f = m.debug_read("part_ffn")
        fvr = t[mf.FFNVR][l * 4 * D: (l + 1) * 4 * D]; fvo = t[mf.FFNVO][l * 4 * D: (l + 1) * 4 * D]
        note("ffn sigmoid(r)", _close(rgate, sig, f"k_ffn_rk layer {l}: sigmoid(ffn_r)"))
        note("ffn relu^2(k)", _close(hbuf, h * fvr, f"k_ffn_rk layer {l}: relu(ffn_k)^2 * ffn_v scale"))
        terms = h.astype(np.float64) * fvo
        assert abs(part_f.sum() - terms.sum()) <= 1e-5 * np.abs(terms).sum(), f"k_ffn_rk layer {l}: offset partials"
        # ---- k_ffnv: x += ffn_v . h * sigmoid(r), state dd = ln2 ----
        vv = oracle.mm8_layer(h, t[mf.FFNV], t[mf.FFNVR], t[mf.FFNVO], 4 * D, D, l)
        x2_ref = x1 + (vv * sig).astype(np.float64)                                                # blockout (rwkv.cu:407): f32 product
        w_fv = t[mf.FFNV].reshape(L, 4 * D, D)[l].astype(np.float64)
        v_contract = (hbuf.astype(np.float64) @ w_fv + part_f.sum()).astype(np.float32)
        x2_contract = x1 + (v_contract * rgate).astype(np.float64)
        m.debug_launch(4, l)
        x2 = m.debug_read("x")
        m.pull_state(n_slots)
        note("ffnv x (oracle)", _close(x2 - x1, x2_ref - x1, f"k_ffnv layer {l}: residual update vs oracle_mm8_one"))
        note("ffnv x (contract)", _close(x2 - x1, x2_contract - x1, f"k_ffnv layer {l}: residual update vs the f64 product of its own input", 1e-5))
        note("ffnv dd", _close(st.statedd[slo], ln2, f"k_ffnv layer {l}: state dd = ln2 output"))
        x = x2
    # ---- k_head: ln_out + head ----
    lno = oracle.layernorm(x[None, :], ln[4 * L + 2: 4 * L + 4])[0]
    logits_ref = oracle.mm8_layer(lno, t[mf.HEAD], t[mf.HEADR], t[mf.HEADO], D, V, 0)
    m.debug_launch(5, 0)
    note("head", _close(m.logits(slot + 1)[slot * V: (slot + 1) * V], logits_ref, "k_head: logits"))              # (logits row = state slot)
    m.pull_state(n_slots)
    for s in range(n_slots):
        if s != slot:
            for name, a, p in zip("xy aa bb pp dd".split(), st.arrays(), pushed):
                assert np.array_equal(a[s * LD: (s + 1) * LD], p[s * LD: (s + 1) * LD]), f"state {name} of slot {s} changed under a token on slot {slot}"
    form = m.decode_form()
    print(f"D={D} L={L} RWKV_TILE={tile} decode_form={form} grid={G} slot={slot}/{n_slots} token={token}: worst {max(worst.values()):.1e}: "
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
