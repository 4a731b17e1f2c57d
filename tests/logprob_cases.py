"""Planted logits rows for the device top-n (csrc/topn.hip.h) and its f64 reference, shared by tests/test_logprobs_cpu.py (no GPU: the
reference held to half the bound against np.longdouble, its tie order pinned) and tests/test_logprobs_gpu.py (the kernels).  TEST
INFRASTRUCTURE: nothing here is imported by the product.

THE REFERENCE (`topn_reference`) is the definition of include/rwkv_mi355x.h in numpy: the n ids with the largest f32 logits in descending
logit order, equal logits by ascending id (a stable sort by (-logit, id) on the f32 values), each with the log-probability of
score_cases.reference.

THE BOUNDS of the device against it: ids equal, no exceptions; |d logprob| <= score_cases.LP_TOL = 1e-10 (where that figure comes from:
score_cases' docstring -- the log-probabilities are the scorer's own); a -inf log-probability exactly -inf.

THE TILING the new rows are planted against is the score tiling, which the top-n part kernel shares (it calls the scorer's slice code): 16
slices [floor(b V / 16), floor((b + 1) V / 16)), each swept by 256 threads in 13 steps -- thread t of slice b holds ids lo(b) + t + 256 k --
and, inside a workgroup, four waves of 64 threads that each select on their own (thread t belongs to wave t // 64).  The kernel has no other
boundary of its own, so no further rows are needed; `one_wave` below adds the wave as the unit that must be able to hand on all n."""
from __future__ import annotations

import functools

import numpy as np

import score_cases as sc

V, LOW = sc.V, sc.LOW
TOPN_MAX = 32
TOP_NS = (1, 2, 5, 20, 32)
SLICES = 16
NEW = ("one_slice", "one_thread", "straddle", "tail", "one_per_slice", "one_wave", "few_finite")
CASES = sc.CASES + NEW


def slice_lo(b):
    return b * V // SLICES


@functools.lru_cache(maxsize=None)
def logits_of(name):
    """the float32 row of a case (read-only, computed once): score_cases' rows, and the rows planted for the selection"""
    if name in sc.CASES:
        return sc.logits_of(name)
    l = np.full(V, LOW, np.float32)
    if name == "one_slice":             # all 32 winners at the head of slice 1 (ids 3142 .. 3173): a per-slice candidate cap below n
        assert slice_lo(1) == 3142
        l[3142:3174] = 10.0 - 0.25 * np.arange(32, dtype=np.float32)
    elif name == "one_thread":          # 13 winners in ONE thread's registers (thread 5 of slice 0), 19 more in threads 6 and 7: a per-thread cap
        ids = [5 + 256 * k for k in range(13)] + [6 + 256 * k for k in range(13)] + [7 + 256 * k for k in range(6)]
        l[ids] = 10.0 - 0.25 * np.arange(32, dtype=np.float32)
    elif name == "one_wave":            # all 32 winners in wave 2 of slice 3 (threads 128 .. 159, step 4), ascending: a per-wave cap, and the order
        lo = slice_lo(3) + 128 + 256 * 4
        l[lo:lo + 32] = 2.0 + 0.25 * np.arange(32, dtype=np.float32)
    elif name == "straddle":            # equal winners on both sides of the boundaries of slices 0|1 and 14|15: the tie rule across slices
        assert slice_lo(1) == 3142 and slice_lo(15) == 47134
        l[[3140, 3141, 3142, 3143, 47133, 47134]] = 3.0
    elif name == "tail":                # an ascending staircase on the last 32 ids: the last, partly filled step of the last slice
        l[V - 32:] = 2.0 + 0.25 * np.arange(32, dtype=np.float32)
    elif name == "one_per_slice":       # one winner per slice, the best one in the LAST slice: the order of the fold
        for b in range(SLICES):
            l[slice_lo(b) + 100 + 7 * b] = 1.0 + 0.5 * b
    elif name == "few_finite":          # three finite logits, -inf everywhere else: from n = 4 on the -inf logits appear, lowest id first, logprob -inf
        l[:] = -np.inf
        l[[7, 3142, V - 1]] = [1.0, 2.5, -3.0]
    else:
        raise KeyError(name)
    l.setflags(write=False)
    return l


def topn_reference(logits, n, dtype=np.float64):
    """(ids [n], logprob [n]) of one row: stable sort by (-logit, id) on the f32 values; the log-probs evaluated in `dtype`"""
    l = np.asarray(logits, np.float32)
    order = np.lexsort((np.arange(l.size), -l.astype(np.float64)))[:n]       # (-l is exact in f64; the last key is the primary one)
    return order.astype(np.int64), sc.reference(l, dtype)[0][order]


@functools.lru_cache(maxsize=None)
def ref_of(name):
    """the f64 reference of a case at n = TOPN_MAX (a smaller n is its prefix): computed once, shared by every test, read-only"""
    ids, lp = topn_reference(logits_of(name), TOPN_MAX)
    ids.setflags(write=False); lp.setflags(write=False)
    return ids, lp


def check(label, got_ids, got_lp, want_ids, want_lp):
    """the bounds, on arrays [.., n]; returns (worst |d logprob|, failures)"""
    got_ids, want_ids = np.asarray(got_ids, np.int64), np.asarray(want_ids, np.int64)
    got_lp, want_lp = np.asarray(got_lp, np.float64), np.asarray(want_lp, np.float64)
    bad = []
    if not np.array_equal(got_ids, want_ids):
        bad.append(f"{label}: ids {got_ids.tolist()} reference {want_ids.tolist()}")
    inf = np.isneginf(want_lp)
    if not np.array_equal(np.isneginf(got_lp), inf):
        bad.append(f"{label}: -inf log-probabilities differ from the reference's")
    with np.errstate(invalid="ignore"):
        d = np.where(inf, 0.0, np.abs(got_lp - want_lp))
    worst = float(np.nanmax(d)) if d.size else 0.0
    if not np.all(d <= sc.LP_TOL):
        bad.append(f"{label}: |d logprob| {worst:.3e} > {sc.LP_TOL}")
    return worst, bad
