"""The planted sampler cases of tests/sampler_cases.py WITHOUT a GPU: (1) the cap on excused draws holds for every case, run and mode from
the reference alone, so that tests/test_sampler_cases_gpu.py cannot hide a failure behind an excuse; (2) the two host restatements --
include/rwkv_sampler.h typical_u (through tests/cpp/sampler_app.cpp) and sampler_recipe.sampler_u -- agree with the log-space reference on
every draw that is not excused, wherever the f64 total of the host weights is a normal number; (3) where those weights all vanish both
return 0 and neither raises."""
import os
import subprocess

import numpy as np
import pytest

import sampler_cases as sc
from sampler_recipe import sampler_u, sampler_weights

from support import build_app

DBL_MIN = 2.2250738585072014e-308

RUNS = sc.all_runs()
IDS = [f"{c.name}-t{temp}-tau{tau}-{'ban0' if ban0 else 'noban'}-{'recipe' if recipe else 'default'}" for (c, temp, tau, ban0, recipe) in RUNS]


@pytest.fixture(scope="module")
def app(tmp_path_factory):
    return build_app("sampler_app", tmp_path_factory.mktemp("sampc"), link=False, opt="-O2")


def banned(name, ban0):
    l = np.array(sc.logits_of(name, ban0), np.float32, copy=True)
    if ban0:
        l[0] = -99.0
    return l


def host_total(l, temp, tau, recipe):
    with np.errstate(under="ignore"):
        return float(sampler_weights(l, temp, tau, recipe).sum())


def app_picks(app, tmp_path, l, temp, tau, recipe, us, vanished=False):
    """typical_u for every u; vanished: exit code 4 is the app's own closing check (a typical() draw has non-zero weight), which cannot hold
    where every weight is zero"""
    path = str(tmp_path / "logits.bin")
    l.tofile(path)
    out = subprocess.run([app, path, repr(temp), repr(tau)] + [repr(u) for u in us], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, RWKV_APP_TRUNCATE="1" if recipe else "0"))
    assert out.returncode in ((0, 4) if vanished else (0,)), out.stderr
    return [int(x) for x in out.stdout.split()]


def test_the_uniforms_are_the_stratified_64_and_both_ends():
    assert len(sc.US) == 66 and sc.US[:2] == (0.5 / 64, 1.5 / 64) and sc.US[-2:] == (0.0, 0.999999999)


@pytest.mark.parametrize("case,temp,tau,ban0,recipe", RUNS, ids=IDS)
def test_at_most_two_draws_are_excused(case, temp, tau, ban0, recipe):
    n = sc.excused_count(case, temp, tau, ban0, recipe)
    print(f"{case.name} temp {temp} tau {tau} ban0 {ban0} recipe {recipe}: {n} of {len(case.us)} excused, eps {sc.ref_of(case.name, temp, tau, ban0, recipe).eps:.3g}")
    assert n <= sc.MAX_EXCUSED


def test_the_tied_cases_hold_what_they_claim():
    for k in (2, 50, 1025):
        for ban0 in (False, True):
            ids = sc.tie_ids(k, ban0)
            l = sc.logits_of(f"d{k}", ban0)
            assert len(ids) == k + (1 if (ban0 and k == 1025) else 0) and 0 in ids and sc.V - 1 in ids
            assert (l[ids] == 0.0).all() and (np.delete(l, ids) == sc.LOW).all()
            if k > 2:
                assert set(sc.EDGE_IDS) <= set(ids.tolist())
            if k == 1025:
                assert set(range(980, 1180)) <= set(ids.tolist())
            # each tied, unbanned token is the pick on its own stretch of u: the middle of stretch j picks the j-th of them
            for recipe in (False, True):
                r = sc.ref_of(f"d{k}", 0.5, sc.TAU, ban0, recipe)
                live = ids[1:] if ban0 else ids
                assert [r.pick((j + 0.5) / len(live)) for j in range(len(live))] == live.tolist()
    p = np.exp(np.float64(sc.LOW)) / 2
    assert p < 1e-30                                       # under the mass skip of the radix select


@pytest.mark.parametrize("case,temp,tau,ban0,recipe", RUNS, ids=IDS)
def test_host_restatements_agree_with_the_reference(app, tmp_path, case, temp, tau, ban0, recipe):
    l = banned(case.name, ban0)
    r = sc.ref_of(case.name, temp, tau, ban0, recipe)
    total = host_total(l, temp, tau, recipe)
    us = list(case.us)
    got_app = app_picks(app, tmp_path, l, temp, tau, recipe, us, vanished=total == 0.0)
    with np.errstate(under="ignore"):
        got_py = sampler_u(l, temp, tau, us, recipe)                       # must not raise, whatever the total
    if total == 0.0:
        # the defined edge of both restatements: every f64 weight vanished -> typical_u's `last`, 0
        assert got_app == [0] * len(us) and got_py == [0] * len(us)
        return
    if not (total >= DBL_MIN and np.isfinite(total)):
        return
    bad = [(u, a, b, r.pick(u)) for u, a, b in zip(us, got_app, got_py) if not r.excused(u) and (a != r.pick(u) or b != r.pick(u))]
    assert not bad, f"(u, typical_u, sampler_u, reference): {bad[:5]}"


def test_the_cases_reach_the_edge_of_the_host_restatements():
    """case b at temp 0.003 is beyond f64 in both modes (the table of cases says so): the branch above that expects 0 is exercised"""
    l = banned("b", False)
    assert host_total(l, 0.003, sc.TAU, False) == 0.0 and host_total(l, 0.003, sc.TAU, True) == 0.0
    assert host_total(l, 0.02, sc.TAU, False) >= DBL_MIN
