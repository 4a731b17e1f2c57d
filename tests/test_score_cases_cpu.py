"""The f64 reference of tests/score_cases.py held to HALF of each bound the device is held to, against the same evaluation in
np.longdouble (x87 80-bit where numpy has it): the reference's own error leaves the device at least half of every tolerance.  Also what
each case is meant to pin: the tie order, the -inf guard, the closed forms.  No GPU."""
import numpy as np
import pytest

import score_cases as sc


@pytest.mark.parametrize("name", sc.CASES)
def test_f64_reference_is_within_half_of_each_bound_of_longdouble(name):
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is no wider than f64 on this platform")
    lp, ent, am = sc.ref_of(name)
    lq, eq, aq = sc.reference(sc.logits_of(name), np.longdouble)
    inf = np.isneginf(lq)
    assert np.array_equal(np.isneginf(lp), inf)
    dl = float(np.max(np.abs(lp.astype(np.longdouble)[~inf] - lq[~inf])))
    de = float(abs(np.longdouble(ent) - eq))
    print(f"{name:>10}: |d logprob| {dl:.2e}  |d entropy| {de:.2e}  entropy {ent:.6f}  argmax {am}")
    assert dl <= sc.LP_TOL / 2 and de <= sc.ENT_TOL / 2 and am == aq
    assert np.isfinite(ent) and not np.isnan(lp).any()


def test_cases_pin_what_they_are_meant_to():
    assert sc.ref_of("ties")[2] == 0 and sc.ref_of("ties_hi")[2] == sc.V - 2 and sc.ref_of("const")[2] == 0
    lp, ent, am = sc.ref_of("const")
    assert np.allclose(lp, -np.log(sc.V), rtol=0, atol=1e-12) and abs(ent - np.log(sc.V)) < 1e-12
    lp, ent, am = sc.ref_of("peak800")
    assert am == 25000 and lp[am] == 0.0 and ent == 0.0 and -812 < lp[0] < -796
    lp, ent, am = sc.ref_of("neginf")
    assert np.isneginf(lp[1::2]).all() and np.isfinite(lp[0::2]).all() and np.isfinite(ent)
    assert abs(sc.ref_of("ties")[1] - np.log(6)) < 1e-9 and abs(sc.ref_of("ties_hi")[1] - np.log(2)) < 1e-9
    lp, ent, am = sc.ref_of("offset1e4")
    assert abs(ent - np.log(sc.V)) < 1e-3


@pytest.mark.parametrize("name", sc.CASES)
def test_targets_cover_the_ends_the_argmax_the_minimum_and_the_last_step(name):
    t = sc.targets_of(name)
    assert all(0 <= g < sc.V for g in t)
    assert {0, 1, sc.V - 1, sc.V - 2, sc.V - 64, 50176, sc.ref_of(name)[2], int(np.argmin(sc.logits_of(name)))} == set(t)
    if name == "neginf":
        assert np.isneginf(sc.ref_of(name)[0][t]).any()          # a -inf target is among them
