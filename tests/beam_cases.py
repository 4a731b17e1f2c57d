"""Planted inputs for the beam-search selection (csrc/beam.hip.h k_beam_select, include/rwkv_sampler.h beam_select) and its brute-force reference,
shared by tests/test_beam_cpu.py (no GPU: the host twin against the reference, the tie order, the margin condition) and tests/test_beam_gpu.py
(the kernels).  TEST INFRASTRUCTURE: nothing here is imported by the product.

A CASE is one step of a width-W search: W logits rows (by name: the rows of tests/logprob_cases.py), the cumulative scores cum [W], the ended flags,
the ids the rows were fed (`last`: an ended row's end token) and the stop ids.  `shifted(case, r)` is the same step with beam j on row (j + r) % W,
so that every row content meets each of the four offsets a logits row can have from a 16-byte boundary (V is odd: row q starts 4 q bytes past one).

THE REFERENCE (`reference`) is the definition of include/rwkv_mi355x.h in numpy, in np.longdouble, WITHOUT the pruning the device relies on: a live row
offers every id 1 .. V - 1 at cum + logprob (score_cases.reference), an ended row its end token at cum; ALL W x 50276 candidates are sorted by
(descending score, ascending parent, the row's own order = descending f32 logit, then ascending id) and the first W are the beams.  That the rows'
top W + 1 hold every winner is thereby tested, not assumed.

THE BOUNDS of the device against it: parents, tokens and ended flags equal, no exceptions; |d score| <= 1e-10 + 2 * 2^-52 * |score| -- the project's
log-prob bound (score_cases.LP_TOL) plus the rounding of the one f64 add and of the reference's own rounding to f64.

THE MARGIN CONDITION makes "equal" decidable: in every case the reference's gap between two neighbours among the first W + 1 candidates is either
exactly 0 by construction (bitwise-equal rows under equal cum, equal logits inside a row, two ended rows at one score) or at least MARGIN = 1e-8,
100 x the log-prob bound: no order here depends on the last bits of a log-probability.  tests/test_beam_cpu.py asserts it for every case and shift."""
from __future__ import annotations

import functools

import numpy as np

import logprob_cases as lc
import score_cases as sc

V = lc.V
MARGIN = 1e-8
SHIFTS = (0, 1, 2, 3)
NINF = -np.inf
_MIX16 = ("flat", "wide", "ties", "ties_hi", "peak800", "neginf", "const", "offset1e4", "one_slice", "one_thread", "straddle", "tail", "one_per_slice",
          "one_wave", "few_finite", "flat")

# name -> (rows, cum, ended, last, stops)
CASES = {
    # bitwise-equal rows under equal cum: W exact ties across parents, ordered by parent
    "equal_w5": (("wide",) * 5, (-3.25,) * 5, (0,) * 5, (1, 2, 3, 4, 5), ()),
    "equal_w16": (("flat",) * 16, (-1.5,) * 16, (0,) * 16, tuple(range(1, 17)), ()),
    # peaked, flat, a -inf half, quantised ties: distinct rows under distinct cum
    "mixed_w5": (("wide", "flat", "peak800", "offset1e4", "neginf"), (-1.0, -2.5, -0.75, -4.0, -3.0), (0,) * 5, (1, 2, 3, 4, 5), ()),
    # one beam far ahead: all W winners from row 1
    "ahead_w5": (("wide", "flat", "peak800", "ties", "neginf"), (-50.0, 0.0, -60.0, -70.0, -80.0), (0,) * 5, (1, 2, 3, 4, 5), ()),
    # the shape of step 0, and -inf between finite entries
    "step0_w5": (("flat",) * 5, (0.0, NINF, NINF, NINF, NINF), (0,) * 5, (9,) * 5, ()),
    "step0_w16": (("wide",) * 16, (0.0,) + (NINF,) * 15, (0,) * 16, (9,) * 16, ()),
    "inf_w5": (("flat", "wide", "neginf", "flat", "ties"), (-1.0, NINF, -2.0, NINF, -3.0), (0,) * 5, (1, 2, 3, 4, 5), ()),
    # ended rows: one candidate each, two of them at one score; a stop id among the winners ends a live beam
    "ended_w5": (("flat", "wide", "ties", "flat", "wide"), (-8.0, -7.5, -9.0, -30.0, -7.5), (0, 1, 0, 0, 1), (11, 222, 3, 4, 555), (49, V - 1)),
    "all_ended_w5": (("flat",) * 5, (-1.0, -2.0, -2.0, -0.5, -4.0), (1,) * 5, (11, 22, 33, 44, V - 1), (7,)),
    # a row whose best id is 0 (dropped), id V - 1 among the winners; every candidate of row 0 at one score, the cut between equal scores
    "id0_w5": (("ties", "const", "ties_hi", "flat", "wide"), (-1.0, -20.0, -30.0, -40.0, -50.0), (0,) * 5, (1, 2, 3, 4, 5), (V - 1,)),
    "const_w5": (("const",) * 5, (-1.0, -1.0, -2.0, -3.0, -4.0), (0,) * 5, (1, 2, 3, 4, 5), ()),
    # W = 2: the second beam and the first loser are equal logits of one row: the row's own order decides
    "cut_w2": (("ties_hi", "wide"), (-1.0, -1.5), (0, 0), (1, 2), (V - 2,)),
    "neginf_w2": (("neginf", "neginf"), (-0.25, -0.5), (0, 0), (1, 2), ()),
    # W = 16 over every planted row, a staircase of cum with an ended row in it
    "mixed_w16": (_MIX16, tuple(-0.5 * j - 0.03125 * (j % 3) for j in range(16)), (0, 0, 0, 1) + (0,) * 12, tuple(range(1, 17)), (3142, V - 1)),
}


def width(name):
    return len(CASES[name][0])


def shifts(name):
    """the shifts a case is run at: W = 5 -- every row content at all four alignments; W = 16 holds its 16 rows at four of each already, W = 2 has
    rows 0 and 1 only: both orders"""
    return SHIFTS if width(name) == 5 else (0, 1)


def case_shifts():
    return [(name, r) for name in CASES for r in shifts(name)]


def shifted(name, r):
    """(rows, cum, ended, last, stops) with beam j on row (j + r) % W"""
    rows, cum, ended, last, stops = CASES[name]
    W = len(rows)
    rot = lambda t: tuple(t[(q - r) % W] for q in range(W))
    return rot(rows), rot(cum), rot(ended), rot(last), stops


@functools.lru_cache(maxsize=None)
def _row(name):
    """of one planted row, computed once: (log-prob of every id in longdouble [V], the place of every id in the row's own order [V])"""
    l = lc.logits_of(name)
    lp = sc.reference(l, np.longdouble)[0]
    order = np.lexsort((np.arange(V), -l.astype(np.float64)))
    place = np.empty(V, np.int64)
    place[order] = np.arange(V)
    return lp, place


@functools.lru_cache(maxsize=None)
def reference(name, r=0):
    """the W beams of a case and shift, by brute force: dict(parent, token, ended [W] int64; score, token_logprob [W] longdouble; sorted [W + 1]
    longdouble: the scores of the first W + 1 candidates)"""
    rows, cum, ended, last, stops = shifted(name, r)
    W = len(rows)
    score, parent, token, place, lps = [], [], [], [], []
    for j in range(W):
        c = np.longdouble(cum[j])
        if ended[j]:
            score.append(np.array([c], np.longdouble)); parent.append(np.array([j])); token.append(np.array([last[j]]))
            place.append(np.array([0])); lps.append(np.array([0.0], np.longdouble))
            continue
        lp, pl = _row(rows[j])
        with np.errstate(invalid="ignore"):
            score.append(c + lp[1:])
        parent.append(np.full(V - 1, j)); token.append(np.arange(1, V)); place.append(pl[1:]); lps.append(lp[1:])
    score, parent, token, place, lps = (np.concatenate(a) for a in (score, parent, token, place, lps))
    assert not np.isnan(score).any()
    first = np.lexsort((place, parent, -score))[: W + 1]                      # (the last key is the primary one)
    win = first[:W]
    was_ended = np.array([ended[j] for j in parent[win]], np.int64)
    out = dict(parent=parent[win].astype(np.int64), token=token[win].astype(np.int64), score=score[win], token_logprob=lps[win],
               ended=(was_ended | np.isin(token[win], list(stops)).astype(np.int64)), sorted=score[first])
    for v in out.values():
        v.setflags(write=False)
    return out


def margins(name, r=0):
    """the gaps between neighbours among the first W + 1 candidates of the reference (longdouble, >= 0; inf where a finite score meets -inf)"""
    s = reference(name, r)["sorted"]
    assert np.isfinite(s[:-1]).all(), "a winner at -inf: its order would rest on nothing"
    return s[:-1] - s[1:]


def rows_topn(rows, n, dtype=np.float64):
    """(ids [W][n], logprob [W][n]) of the rows of a case: what rwkv_topn_rows returns for them, from the numpy reference"""
    refs = [_row_topn(q, n, dtype) for q in rows]
    return np.stack([a[0] for a in refs]), np.stack([np.asarray(a[1], np.float64) for a in refs])


@functools.lru_cache(maxsize=None)
def _row_topn(name, n, dtype):
    return lc.topn_reference(lc.logits_of(name), n, dtype)


def score_tol(score):
    return sc.LP_TOL + 2.0 * 2.0 ** -52 * np.abs(np.asarray(score, np.float64))


def check(label, got, want):
    """the bounds: got = (parent, token, score, token_logprob, ended) of the device or the host twin, want = reference(...); returns
    (worst |d score|, failures)"""
    parent, token, score, lp, ended = got
    bad = []
    for key, g in (("parent", parent), ("token", token), ("ended", ended)):
        if not np.array_equal(np.asarray(g, np.int64), want[key]):
            bad.append(f"{label}: {key} {np.asarray(g).tolist()} reference {want[key].tolist()}")
    ws = want["score"].astype(np.float64)
    d = np.abs((np.asarray(score, np.float64).astype(np.longdouble) - want["score"]).astype(np.float64))
    dl = np.abs((np.asarray(lp, np.float64).astype(np.longdouble) - want["token_logprob"]).astype(np.float64))
    worst = float(d.max())
    if not np.all(d <= score_tol(ws)):
        bad.append(f"{label}: |d score| {worst:.3e} above 1e-10 + 2 ulp")
    if not np.all(dl <= sc.LP_TOL):
        bad.append(f"{label}: |d token logprob| {float(dl.max()):.3e} > {sc.LP_TOL}")
    return worst, bad
