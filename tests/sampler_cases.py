"""Planted logits for the device sampler (csrc/sampler.hip.h) and a log-space f64 reference of the draw, shared by
tests/test_sampler_cases_cpu.py (no GPU: the cap on excused draws, the two host restatements against the reference) and
tests/test_sampler_cases_gpu.py (the kernels).  TEST INFRASTRUCTURE: nothing here is imported by the product.

THE REFERENCE (`reference`) evaluates typical_weights / typical_u of include/rwkv_sampler.h in log space, so that it has no underflow
of its own: log p_i = l_i - M - log Z; the entropy over the terms with p_i > 0; the key |-log p_i - H|; the kept set as typical_weights
defines it (stable order of keys, smallest prefix whose mass reaches tau, every token with key <= the cutoff key; default mode keeps
everything); log-weights expo * log p_i on the kept set with expo as make_sampler of csrc/engine.hip derives it (temp == 1 -> 1, default
mode n = uint8(1 / temp) clamped at 255, n = 0 -> every weight 1); weights exp(lw - max lw); inverse CDF in token order.

WHEN A DRAW IS EXCUSED (`Ref.excused`, from the reference alone).  A STEP is a point of [0, 1) where the reference's pick changes: the
normalised running sum behind every token of non-zero weight but the last (0 and 1 are no steps: u >= 0 picks the first such token, u < 1
the last).  A draw is excused when u lies within `Ref.eps` of a step;
    eps = EPS + 2 delta,     EPS = 1e-6 (the device's f32 weights carry 6e-8 relative error each; 1e-6 covers a 50 k-term sum),
where delta measures how far the kept set of recipe mode is ambiguous: K_lo is the kept set with the cut taken where the mass reaches
tau - TAU_EPS, K_hi the one with the cut where it reaches tau + TAU_EPS and every token whose key exceeds that cutoff key by less than
2^-22 relative (f32 keys tie there) taken in as well; delta = weight(K_hi \\ K_lo) / weight(K_lo).  Every kept set K between the two has
a normalised CDF within 2 delta of the reference's, and a token of K_hi \\ K_lo owns a stretch of at most delta, so a u further than eps
from every step has the same pick under every such K.  This excuses NO MORE than excusing every draw of an ambiguous pair would (delta = 0
where nothing is ambiguous), and it keeps pairs testable whose ambiguity is structural and harmless: tau = 1.0 always lies within any
tolerance of the mass of the tail of the distribution, which carries next to no weight.
TAU_EPS = 2^-23, not 1e-6: the device adds up f32(p_i) in f64, each within 2^-24 relative of p_i, so its running mass is within 2^-24 of
the reference's (the masses sum to 1); twice that is allowed.  At 1e-6 case a at (2.0, 0.999) could not be tested in recipe mode with any
seed: ~20 tail tokens of p ~ 1e-7 lie within 1e-6 of the cut, temp = 2 raises each to 3e-4 of the total weight, and the steps of the
20 000 kept tokens are 5e-5 apart.  The tighter figure excuses less.
With expo = 0 (default mode, temp > 1) every weight is exactly 1 on both sides, every partial sum an integer and u * total rounded once:
eps = 0 there, nothing is excused.  (At 1 / 50277 per token and u = (i + 0.5) / 64, six of the 64 draws lie within 1e-6 of a step by
arithmetic, for every seed.)

THE CAP: per case, run and mode at most MAX_EXCUSED = 2 of the draws are excused (asserted by the CPU test for every one of them; the seeds
below were searched for it: with ~15 000 tokens owning more than 2e-6 each, a flat case excuses ~2 of 64 stratified draws on average).

TWO PLACES where a case differs from its one-line description, both forced by the cap:
  * d1025 with ban0: 1024 unbanned ties put every stratified u = (16 i + 8) / 1024 exactly ON a step.  One more id joins the tie in the ban0
    run (1026 tied, 1025 unbanned).
  * d2 holds ids 0 and V - 1 only (two ids cannot include six)."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

V = 50277
EPS = 1e-6
KEY_TIE = 2.0 ** -22
TAU_EPS = 2.0 ** -23
MAX_EXCUSED = 2
US = tuple((i + 0.5) / 64 for i in range(64)) + (0.0, 0.999999999)
LOW = -80.0                      # the logit of everything outside a planted tie: p ~ 1e-35, under the 1e-30 skip of the radix select
EDGE_IDS = (0, 1, 49, 50, 51, V - 1)   # first / last token, both sides of the first 50-token ownership boundary


def expo_of(temp, recipe):
    """make_sampler (csrc/engine.hip): the exponent applied to p"""
    t = np.float32(temp)
    if t == np.float32(1.0):
        return 1.0
    e = 1.0 / float(t)
    if recipe:
        return e
    return 255.0 if e >= 255.0 else float(int(e))


@dataclass
class Ref:
    w: np.ndarray          # weights relative to the largest kept one (0 outside the kept set)
    c: np.ndarray          # running sum of w in token order
    steps: np.ndarray      # normalised positions where the pick changes, ascending
    eps: float
    last: int              # the last token of non-zero weight

    def pick(self, u):
        i = int(np.searchsorted(self.c, u * self.c[-1], side="right"))
        return i if i < len(self.w) else self.last

    def excused(self, u):
        if self.eps <= 0.0 or not len(self.steps):
            return False
        j = int(np.searchsorted(self.steps, u))
        near = [abs(self.steps[k] - u) for k in (j - 1, j) if 0 <= k < len(self.steps)]
        return bool(min(near) < self.eps)


def reference(logits, temp, tau, recipe, ban0=False):
    l = np.array(logits, np.float32, copy=True).astype(np.float64)
    if ban0:
        l[0] = -99.0
    n = len(l)
    M = l.max()
    logp = l - M - np.log(np.exp(l - M).sum())
    p = np.exp(logp)
    pos = p > 0
    H = -(p[pos] * logp[pos]).sum()
    key = np.abs(-logp - H)
    expo = expo_of(temp, recipe)
    lw = expo * logp if expo != 0.0 else np.zeros(n)
    delta = 0.0
    if recipe:
        ids = np.argsort(key, kind="stable")
        cum = np.cumsum(p[ids])
        tauf = float(np.float32(tau))
        cut = lambda t: key[ids[min(int((cum < t).sum()), n - 1)]]
        kept = key <= cut(tauf)
        k_lo = key <= cut(tauf - TAU_EPS)
        k_hi = key <= cut(tauf + TAU_EPS) * (1.0 + KEY_TIE)
        mx = lw[kept].max()
        with np.errstate(over="ignore"):
            delta = float(np.exp(lw[k_hi & ~k_lo] - mx).sum() / np.exp(lw[k_lo] - mx).sum())
    else:
        kept = np.ones(n, bool)
        mx = lw.max()
    w = np.where(kept, np.exp(np.where(kept, lw - mx, -np.inf)), 0.0)
    c = np.cumsum(w)
    nz = np.nonzero(w > 0)[0]
    eps = 0.0 if expo == 0.0 else EPS + 2.0 * delta
    return Ref(w=w, c=c, steps=c[nz[:-1]] / c[-1], eps=eps, last=int(nz[-1]))


# ---- the cases ------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    runs: tuple            # (temp, tau, ban0)
    modes: tuple = (False, True)     # recipe
    us: tuple = US


# seeds: searched (lowest first) for the cap over every run and mode of the case; c also for p_max < 0.3 (0.16), so that p_max^n is below
# f32 at every temp of the case (p_max < 0.36 at temp 0.01; seeds 0 .. 5 have one token above that)
SEEDS = dict(a=31, b=28, c=6, d=0, e=5, h=1)

TAU = 0.8
CASES = {c.name: c for c in (
    Case("a", ((0.9, 0.8, False), (1.0, 0.95, False), (0.5, 0.2, False), (2.0, 0.999, False))),
    Case("b", tuple((t, TAU, False) for t in (0.3, 0.1, 0.06, 0.02, 0.003))),          # n = 3, 10, 16, 50, 255
    Case("c", tuple((t, TAU, False) for t in (0.04, 0.02, 0.01, 0.004))),              # n = 25, 50, 100, 250
    Case("d2", ((0.5, TAU, False), (0.5, TAU, True))),
    Case("d50", ((0.5, TAU, False), (0.5, TAU, True))),
    Case("d1025", ((0.5, TAU, False), (0.5, TAU, True))),
    Case("e", ((1.0, 0.5, False), (1.0, 1.5, False), (2.0, 0.5, False), (2.0, 1.5, False))),
    Case("f", ((1.0, 0.5, True), (2.0, 0.5, True))),
    Case("g", ((1.0, TAU, False), (0.5, TAU, False)), us=(0.0, 0.5, 0.999999999)),
    Case("h", tuple((t, tau, False) for t in (1.0, 0.5) for tau in (0.0, 1e-12, 1.0, 1.5)), modes=(True,)),
)}
ROW_CASES = ("c", "d50", "g")        # case r: planted together in rows 0, 1 and the last row, then rotated once


def _normal(name, scale):
    return (scale * np.random.default_rng(SEEDS[name]).standard_normal(V)).astype(np.float32)


def tie_ids(k, ban0):
    """the ids tied at the top of case d<k>"""
    if k == 2:
        return np.array([0, V - 1])
    ids = set(EDGE_IDS)
    if k > 1000:
        ids |= set(range(980, 1180))          # a run over the owners 19 .. 23 of k_typical (50 tokens each)
    want = k + (1 if (ban0 and k == 1025) else 0)
    for t in np.random.default_rng(SEEDS["d"] + k).permutation(V):
        if len(ids) >= want:
            break
        ids.add(int(t))
    return np.array(sorted(ids))


@functools.lru_cache(maxsize=None)
def logits_of(name, ban0=False):
    """the float32 vector of a case (ban0 only selects the tie set of d1025; the ban itself is applied by the sampler)"""
    if name == "a" or name == "h":
        l = _normal(name, 4.0)
    elif name == "b":
        l = _normal(name, 1.0)
    elif name == "c":
        l = _normal(name, 8.0)
    elif name[0] == "d":
        l = np.full(V, LOW, np.float32)
        l[tie_ids(int(name[1:]), ban0)] = 0.0
    elif name == "e":
        l = (np.random.default_rng(SEEDS["e"]).standard_normal(V)).astype(np.float32)
        l[25000] = l.max() + 800.0
    elif name == "f":
        l = np.full(V, -900.0, np.float32)
        l[0] = 5.0
    elif name == "g":
        l = np.full(V, LOW, np.float32)
        l[[V - 2, V - 1]] = 0.0
    else:
        raise KeyError(name)
    l.setflags(write=False)
    return l


@functools.lru_cache(maxsize=None)
def ref_of(name, temp, tau, ban0, recipe):
    """the reference of one case, run and mode: computed once, shared by every test"""
    return reference(logits_of(name, ban0), temp, tau, recipe, ban0)


def all_runs():
    """(case, temp, tau, ban0, recipe) of every case, run and mode"""
    return [(c, temp, tau, ban0, recipe) for c in CASES.values() for (temp, tau, ban0) in c.runs for recipe in c.modes]


def excused_count(case, temp, tau, ban0, recipe):
    r = ref_of(case.name, temp, tau, ban0, recipe)
    return sum(r.excused(u) for u in case.us)


def splitmix_u(seed, step):
    """the uniform of (seed, step) in the device-side generation loops (csrc/sampler.hip.h)"""
    m = (1 << 64) - 1
    x = (seed + step + 0x9E3779B97F4A7C15) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    x ^= x >> 31
    return (x >> 11) / 9007199254740992.0


def logits_view(m, rows=1):
    """the engine's device logits buffer, rows 0 .. rows - 1, as a torch tensor [rows][V]: to plant chosen logits vectors"""
    import torch
    from rwkv_cpp_accelerated_amd import engine

    class _A:
        __cuda_array_interface__ = dict(shape=(int(rows), V), typestr="<f4", data=(int(engine.lib().rwkv_logits_device(m._h)), False), version=2)
    return torch.as_tensor(_A(), device="cuda:0")
