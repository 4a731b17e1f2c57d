"""Planted logits rows for the device scorer (csrc/score.hip.h) and its f64 reference, shared by tests/test_score_cases_cpu.py (no GPU:
the reference held to half of each bound against np.longdouble) and tests/test_score_gpu.py (the kernels).  TEST INFRASTRUCTURE: nothing
here is imported by the product.

THE REFERENCE (`reference`) is the definition of include/rwkv_mi355x.h in numpy: with l_i the f32 logits widened to the working type,
M = max l_i, d_i = l_i - M, Z = sum exp(d_i):
    logprob_g = d_g - log Z                                        (-inf for a target whose logit is -inf)
    entropy   = log Z - (sum_{i: d_i > -inf} exp(d_i) d_i) / Z     (a -inf logit contributes 0, not 0 * inf)
    argmax    = the lowest id with l_i == M

THE BOUNDS of the device against the f64 reference: |d logprob| <= LP_TOL = 1e-10, |d entropy| <= ENT_TOL = 1e-9, argmax equal, a -inf
log-probability exactly -inf.  Re-ordering a 50 277-term f64 sum moves it by at most V 2^-53 = 5.6e-12 relative; exp and log add a few ulp;
the subtraction d_g - log Z at magnitude 800 adds 2e-13; the entropy is at most log V = 10.83 nats times that relative error, all terms of
sum e d being of one sign.  An implementation that accumulates in f32 misses by four orders of magnitude."""
from __future__ import annotations

import functools

import numpy as np

V = 50277
LP_TOL, ENT_TOL = 1e-10, 1e-9
LOW = -80.0
TIE_IDS = (0, 1, 49, 50, 51, V - 1)
CONST = -7.25                    # every logit of case `const` (negative: the maximum of a row need not be positive)
CASES = ("flat", "wide", "ties", "ties_hi", "peak800", "neginf", "const", "offset1e4")
SEEDS = dict(flat=1, wide=2, peak800=3, neginf=4, offset1e4=5)


def _normal(name, scale):
    return (scale * np.random.default_rng(SEEDS[name]).standard_normal(V)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def logits_of(name):
    """the float32 row of a case (read-only, computed once)"""
    if name == "flat":
        l = _normal(name, 1.0)
    elif name == "wide":
        l = _normal(name, 30.0)
    elif name == "ties":
        l = np.full(V, LOW, np.float32)
        l[list(TIE_IDS)] = 3.0
    elif name == "ties_hi":
        l = np.full(V, LOW, np.float32)
        l[[V - 2, V - 1]] = 3.0
    elif name == "peak800":
        l = _normal(name, 1.0)
        l[25000] = l.max() + np.float32(800.0)
    elif name == "neginf":
        l = _normal(name, 1.0)
        l[1::2] = -np.inf
    elif name == "const":
        l = np.full(V, CONST, np.float32)
    elif name == "offset1e4":
        l = (1e4 + 1e-3 * np.random.default_rng(SEEDS[name]).standard_normal(V)).astype(np.float32)
    else:
        raise KeyError(name)
    l.setflags(write=False)
    return l


def reference(logits, dtype=np.float64):
    """(logprob of EVERY id [V], entropy, argmax) of one row, evaluated in `dtype`"""
    l = np.asarray(logits, np.float32).astype(dtype)
    M = l.max()
    d = l - M
    e = np.exp(d)
    Z = e.sum()
    logZ = np.log(Z)
    fin = d > -np.inf
    ent = logZ - (e[fin] * d[fin]).sum() / Z
    return d - logZ, ent, int(np.argmax(l == M))


@functools.lru_cache(maxsize=None)
def ref_of(name):
    """the f64 reference of a case: computed once, shared by every test, read-only"""
    lp, ent, am = reference(logits_of(name))
    lp.setflags(write=False)
    return lp, float(ent), am


def targets_of(name):
    """the ids scored in a case: both ends, the argmax, the minimum, and ids in the last, partly filled step of a tiling of the row (the last
    slice of the 16 the kernel makes starts at 47134; 50176 = 196 * 256 is where a 256-thread sweep of the whole row has its last step)"""
    l = logits_of(name)
    return [0, 1, V - 1, ref_of(name)[2], int(np.argmin(l)), V - 2, V - 64, 50176]


def check(label, got_lp, got_ent, got_am, want_lp, want_ent, want_am):
    """the bounds, on arrays of queries; returns (worst |d logprob|, worst |d entropy|, failures)"""
    got_lp, want_lp = np.asarray(got_lp, np.float64), np.asarray(want_lp, np.float64)
    got_ent, want_ent = np.asarray(got_ent, np.float64), np.asarray(want_ent, np.float64)
    bad = []
    inf = np.isneginf(want_lp)
    if not np.array_equal(np.isneginf(got_lp), inf):
        bad.append(f"{label}: -inf log-probabilities at {np.nonzero(np.isneginf(got_lp))[0].tolist()}, reference at {np.nonzero(inf)[0].tolist()}")
    with np.errstate(invalid="ignore"):
        dlp = np.where(inf, 0.0, np.abs(got_lp - want_lp))
    dent = np.abs(got_ent - want_ent)
    wl, we = (float(np.nanmax(dlp)) if dlp.size else 0.0), (float(np.nanmax(dent)) if dent.size else 0.0)
    if not (np.all(dlp <= LP_TOL)):
        bad.append(f"{label}: |d logprob| {wl:.3e} > {LP_TOL}")
    if not (np.all(dent <= ENT_TOL)):
        bad.append(f"{label}: |d entropy| {we:.3e} > {ENT_TOL}")
    if not np.array_equal(np.asarray(got_am, np.int64), np.asarray(want_am, np.int64)):
        bad.append(f"{label}: argmax {np.asarray(got_am).tolist()} reference {np.asarray(want_am).tolist()}")
    return wl, we, bad
