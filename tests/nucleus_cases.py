"""Planted logits and occurrence counts for the device nucleus sampler (csrc/nucleus.hip.h) and a log-space f64 reference of its draw, shared by
tests/test_nucleus_cpu.py (no GPU: the cap on excused draws, a literal numpy transcription and the host twin against the reference) and
tests/test_nucleus_gpu.py (the kernels and the loops).  TEST INFRASTRUCTURE, modelled on tests/sampler_cases.py, whose draws (US), tie sets,
Ref (pick / excused) and splitmix generator it shares: nothing here is imported by the product.

THE REFERENCE (`reference`) restates the semantics of include/rwkv_mi355x.h (rwkv_sample_nucleus) in f64:
    l'_i = l_i - (presence + c_i frequency) where c_i > 0 (every factor an f32 widened to f64), l'_0 = -99 under the ban, afterwards;
    log p_i = l'_i - M - log sum exp(l' - M); key_i = -log p_i; order = stable argsort of the key (descending p, stable in token id);
    top-p cut key = the key at the first position where the running mass reaches top_p (no such position: the largest key, everything is
    kept; top_p <= 0: the smallest); top-k cut key = the top_k-th smallest key (0 < top_k < V, else none); kept = key <= both cut keys;
    weights exp((l'_i - M) / temp) on the kept set (temp == 1: the exponent is l'_i - M itself); inverse CDF in token order.

WHEN A DRAW IS EXCUSED (sampler_cases.Ref.excused, from the reference alone): u lies within eps = 1e-6 + 2 delta of a step of the reference's
CDF.  delta = weight(K_hi \\ K_lo) / weight(K_lo) measures how far the kept set is ambiguous on a device that adds up f32(p_i) and compares
f32 keys: K_lo is the kept set with the top-p cut taken at top_p - 2^-23, K_hi the one with the cut at top_p + 2^-23 and every token whose
key is within 2^-22 relative of either cut key (top-p's or top-k's: f32 keys tie there) taken in as well.  sampler_cases' docstring has the
argument for these figures; it carries over because the select is the same.  An f32 tie can only ADD tokens at the top-k cut (rounding is
monotone: whatever is <= the top_k-th key in f64 is in f32), so K_lo takes the top-k cut as it is.

THE CAP: per case and run at most MAX_EXCUSED = 2 of the 66 draws are excused (asserted by the CPU test for every run; seeds searched for it).
(temp 2, top_p 0.999) on case a is left out: 28 of 66 draws are ambiguous by construction -- the tail near that cut is dense and temp 2 makes
it heavy."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import sampler_cases as sc
from sampler_cases import EDGE_IDS, LOW, MAX_EXCUSED, US, V, Ref, logits_view, splitmix_u  # noqa: F401  (shared with the tests)

EPS = 1e-6
KEY_TIE = 2.0 ** -22
TOP_P_EPS = 2.0 ** -23
PEN_COUNTS = (1, 2, 3, 20.5, 1, 0.996, 7, 1, 1, 2, 0.5, 40)     # planted on the twelve largest logits of a case


def penalised(logits, counts, presence, frequency, ban0):
    """l' in f64"""
    l = np.array(logits, np.float32, copy=True).astype(np.float64)
    pr, fr = float(np.float32(presence)), float(np.float32(frequency))
    if pr != 0.0 or fr != 0.0:
        c = np.asarray(counts, np.float32).astype(np.float64)
        l = np.where(c > 0, l - (pr + c * fr), l)
    if ban0:
        l[0] = -99.0
    return l


def reference(logits, temp, top_p, top_k=0, counts=None, presence=0.0, frequency=0.0, ban0=False) -> Ref:
    l = penalised(logits, counts, presence, frequency, ban0)
    n = len(l)
    M = l.max()
    logp = l - M - np.log(np.exp(l - M).sum())
    p = np.exp(logp)
    key = -logp
    ids = np.argsort(key, kind="stable")
    cum = np.cumsum(p[ids])
    tp = float(np.float32(top_p))
    cut = lambda t: key[ids[min(int((cum < t).sum()), n - 1)]]
    k = int(top_k)
    cut_k = key[ids[k - 1]] if 0 < k < n else np.inf
    kept = key <= min(cut(tp), cut_k)
    k_lo = key <= min(cut(tp - TOP_P_EPS), cut_k)
    k_hi = key <= min(cut(tp + TOP_P_EPS), cut_k) * (1.0 + KEY_TIE)
    t = float(np.float32(temp))
    lw = (l - M) if t == 1.0 else (l - M) / t
    delta = float(np.exp(lw[k_hi & ~k_lo]).sum() / np.exp(lw[k_lo]).sum())
    w = np.where(kept, np.exp(np.where(kept, lw, -np.inf)), 0.0)
    c = np.cumsum(w)
    nz = np.nonzero(w > 0)[0]
    return Ref(w=w, c=c, steps=c[nz[:-1]] / c[-1], eps=EPS + 2.0 * delta, last=int(nz[-1]))


def count_update(counts, pick, decay):
    """the count update in f32, as the device does it: f32(c decay) for every token, then + 1 for the pick (decay 1: no multiply)"""
    c = np.asarray(counts, np.float32)
    d = np.float32(decay)
    c = c.copy() if d == np.float32(1.0) else (c * d).astype(np.float32)
    c[pick] = np.float32(c[pick] + np.float32(1.0))
    return c


# ---- the cases ------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Run:
    temp: float
    top_p: float
    top_k: int = 0
    ban0: bool = False
    presence: float = 0.0
    frequency: float = 0.0


@dataclass(frozen=True)
class Case:
    name: str
    logits: str            # key of logits_of
    runs: tuple
    counted: bool = False  # PEN_COUNTS planted on the twelve largest logits


SEEDS = dict(a=1, b=4, c=sc.SEEDS["c"])      # c: p_max < 0.3, 13 tokens kept at top_p 0.8
SCALE = dict(a=4.0, b=1.0, c=8.0)

_TIES = tuple(Run(0.5, tp, tk, ban) for ban in (False, True) for (tp, tk) in ((0.5, 0), (1.0, 3)))
CASES = {c.name: c for c in (
    Case("a", "a", tuple(Run(*r) for r in ((1, 0.9, 0), (0.7, 0.5, 0), (2, 0.9, 0), (1.5, 0.99, 0), (1, 0.1, 0), (1, 1, 40), (0.5, 0.95, 1000),
                                           (1, 0, 0), (1, 1, 0), (1, 0.9, 1), (2, 1.5, V)))),
    Case("b", "b", tuple(Run(t, 0.8) for t in (0.3, 0.1, 0.06, 0.02, 0.01)) + (Run(1, 0.5, 5000),)),
    Case("c", "c", tuple(Run(t, 0.8) for t in (0.04, 0.02, 0.01, 0.004))),
    Case("d2", "d2", _TIES),
    Case("d50", "d50", _TIES),
    Case("d1025", "d1025", _TIES),
    Case("e", "e", (Run(1, 0.5), Run(2, 1.5), Run(1, 0.9, 40))),                 # one token 800 above the rest
    Case("f", "f", (Run(1, 0.5, 0, True), Run(2, 0.9, 40, True))),              # all at -900 except id 0, under the ban: -99 still is the largest
    Case("p", "a", tuple(Run(t, tp, tk, False, pr, fr) for (pr, fr) in ((0.4, 0.4), (5, 2)) for (t, tp, tk) in ((1, 0.9, 0), (0.7, 0.5, 40))), counted=True),
)}
# case r: three rows of different content, each sampled with the counts of a different slot: (case whose logits the row holds, row, slot)
ROW_CASE = (("a", 0, 2), ("c", 1, 0), ("d50", 3, 1))      # (d50: the counts fall on twelve of the fifty tied ids and split the tie)
ROW_RUNS = (Run(1, 0.9, 0, False, 0.4, 0.4), Run(0.7, 0.5, 40, True, 5, 2))


@functools.lru_cache(maxsize=None)
def logits_of(name, ban0=False):
    """the float32 vector of a case (ban0 only selects the tie set of d1025, as in sampler_cases; the ban itself is applied by the sampler)"""
    if name in SEEDS:
        l = (SCALE[name] * np.random.default_rng(SEEDS[name]).standard_normal(V)).astype(np.float32)
        l.setflags(write=False)
        return l
    return sc.logits_of(name, ban0)


@functools.lru_cache(maxsize=None)
def counts_of(name, shift=0):
    """PEN_COUNTS (rotated by `shift`) on the twelve largest logits of `name`, zero elsewhere"""
    c = np.zeros(V, np.float32)
    top = np.argsort(-logits_of(name).astype(np.float64), kind="stable")[: len(PEN_COUNTS)]
    c[top] = np.roll(np.array(PEN_COUNTS, np.float32), shift)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def ref_of(lname, run, counted=False, shift=0):
    """the reference of one run on the logits `lname`, with PEN_COUNTS rotated by `shift` planted if `counted`: computed once, shared by every test"""
    return reference(logits_of(lname, run.ban0), run.temp, run.top_p, run.top_k, counts_of(lname, shift) if counted else None,
                     run.presence, run.frequency, run.ban0)


def all_runs():
    """(label, logits name, run, counted, count rotation) of every case and run, the row case included"""
    out = [(c.name, c.logits, r, c.counted, 0) for c in CASES.values() for r in c.runs]
    return out + [(f"r/{n}", n, r, True, slot) for (n, _, slot) in ROW_CASE for r in ROW_RUNS]


def excused_count(lname, run, counted=False, shift=0):
    r = ref_of(lname, run, counted, shift)
    return sum(r.excused(u) for u in US)
