"""The device sampler (csrc/sampler.hip.h: k_typical_stats, k_typical_keys, k_typical) on the planted logits of tests/sampler_cases.py,
draw by draw against the log-space f64 reference there.  A device pick that differs from the reference's is a failure unless the reference
alone excuses the draw (sampler_cases.Ref.excused; tests/test_sampler_cases_cpu.py caps the excused draws at 2 per case, run and mode).
Every run prints its tally (draws, excused, mismatched) before anything is asserted.

Measured on an MI355X with the sampler as it was before its weights were formed relative to the largest one (p^expo as an f32: zero for
EVERY token once p_max^expo < 1.4e-45, the pick then fell through to id 0): case b failed at temp 0.06, 0.02 and 0.003 and case c at 0.01
and 0.004, in both modes, 64 or 65 of the 66 draws each; case r failed in the rows that held case c, before and after the rotation, likewise;
decode_typical and decode_batch_typical at temp 0.01 returned id 0 at steps 4, 6 and 8 of the stream from token 30000.  Every other case and run
passed there
(profiles/NOTES.md, "sampler on planted logits").  Now: no mismatched draw in any run."""
import numpy as np
import pytest

import sampler_cases as sc
from support import eng, load, plant_rows  # noqa: F401

from rwkv_cpp_accelerated_amd import modelfile as mf

pytestmark = pytest.mark.gpu

ROWS = 4                      # maxGPT of the planted context: rows 0, 1 and 3 (the last) are used


@pytest.fixture(scope="module")
def ctx(eng):
    m = load(eng, 2, 64, 3, ROWS)
    m.forward(5)
    yield m
    m.close()


def run_case(m, name, row, label):
    """every run, mode and u of case `name` on logits row `row` (planted by the caller); returns the failures, prints the tallies"""
    case, bad = sc.CASES[name], []
    for (temp, tau, ban0) in case.runs:
        if name == "d1025" and ban0:
            plant_rows(m, {row: sc.logits_of(name, True)}, ROWS)         # (its tie set has one more id under ban0: sampler_cases' docstring)
        for recipe in case.modes:
            r = sc.ref_of(name, temp, tau, ban0, recipe)
            excused = mismatched = 0
            for u in case.us:
                got = m.sample_typical(temp, tau, u, row=row, ban0=ban0, recipe=recipe)
                want = r.pick(u)
                ex = r.excused(u)
                excused += ex
                why = None
                if got >= sc.V:
                    why = "pick outside the vocabulary"
                elif ban0 and got == 0 and want != 0:
                    # id 0 under ban0 is right only where the reference picks it too: case f (-99 still dominates -900) and temp > 1 in default
                    # mode, where nc::power(p, 0) = 1 gives the banned token the weight of every other one (typical.h:52) -- mirrored, not excused
                    why = "the banned id 0"
                elif got != want and not ex:
                    why = "differs from the reference"
                if why:
                    mismatched += 1
                    bad.append((label, temp, tau, ban0, recipe, u, got, want, why))
            print(f"{label:>8} temp {temp:<5} tau {tau:<5} ban0 {int(ban0)} {'recipe ' if recipe else 'default'}: draws {len(case.us)} excused {excused} mismatched {mismatched}")
    return bad


@pytest.mark.parametrize("name", list(sc.CASES))
def test_planted_case_matches_the_log_space_reference(ctx, name):
    plant_rows(ctx, {0: sc.logits_of(name, False)}, ROWS)
    bad = run_case(ctx, name, 0, name)
    assert not bad, f"{len(bad)} draws, first (case, temp, tau, ban0, recipe, u, device, reference, why): {bad[:4]}"


def test_rows_are_addressed_one_by_one_case_r(ctx):
    """rows 0, 1 and the last hold three different distributions at once; each is sampled with row = r; then the contents rotate"""
    where = (0, 1, ROWS - 1)
    bad = []
    for shift in (0, 1):
        names = [sc.ROW_CASES[(k - shift) % 3] for k in range(3)]
        plant_rows(ctx, {r: sc.logits_of(n, False) for r, n in zip(where, names)}, ROWS)
        for r, n in zip(where, names):
            bad += run_case(ctx, n, r, f"r{shift}/{n}@{r}")
    assert not bad, f"{len(bad)} draws, first (case, temp, tau, ban0, recipe, u, device, reference, why): {bad[:4]}"


# ---- the fix reaches the generation loops: near-greedy temperature on a model's own logits ---------------------------------------------
L, D, N_GEN, TEMP, TAU = 2, 256, 16, 0.01, 0.8


@pytest.fixture(scope="module")
def model(eng):
    m = load(eng, L, D, 12, ROWS, head_scale=30.0)
    yield m
    m.close()


def follow(logits, u, got, recipe, where):
    """the reference's pick for this step; the device's where the draw is excused (and only there)"""
    r = sc.reference(logits, TEMP, TAU, recipe, ban0=True)
    want = r.pick(u)
    if want != got:
        assert r.excused(u), f"{where}: device {got} reference {want} (u {u!r})"
        want = got
    return want


@pytest.mark.parametrize("recipe", [False, True])
def test_decode_typical_near_greedy_equals_the_reference_loop(model, recipe):
    m, first, seed = model, 30000, 33        # the third stream of the batched test below: p_max^100 is below f32 at three of its 16 steps
    m.reset_state()
    ids = [int(v) for v in m.decode_typical(first, N_GEN, temp=TEMP, tau=TAU, seed=seed, recipe=recipe)]
    print("decode_typical", "recipe" if recipe else "default", ids)
    m.reset_state()
    tk = first
    for step in range(N_GEN):
        logits = m.forward(tk)[: mf.VOCAB].copy()
        tk = follow(logits, sc.splitmix_u(seed, step), ids[step], recipe, f"step {step}")
    assert all(0 < v < mf.VOCAB for v in ids)


@pytest.mark.parametrize("recipe", [False, True])
def test_decode_batch_typical_near_greedy_equals_the_reference_loop(eng, model, recipe):
    m, first, seeds = model, [9, 4242, 30000], [11, 22, 33]
    m.reset_state()
    got = m.decode_batch_typical(first, N_GEN, temp=TEMP, tau=TAU, seeds=seeds, recipe=recipe).astype(np.int64)
    print("decode_batch_typical", "recipe" if recipe else "default", got.tolist())
    m.reset_state()
    ids = list(first)
    for step in range(N_GEN):
        lg = m.forward(ids, eng.MODE_PARRALEL)[: 3 * mf.VOCAB].reshape(3, mf.VOCAB).copy()
        ids = [follow(lg[s], sc.splitmix_u(seeds[s], step), int(got[s, step]), recipe, f"stream {s} step {step}") for s in range(3)]
    assert ((got > 0) & (got < mf.VOCAB)).all()
