"""The f64 numpy reference of the device's floor samplers (csrc/floor.hip.h), restated from include/rwkv_mi355x.h (rwkv_sample_floor), and their
parameter runs on the planted logits of tests/nucleus_cases.py.  TEST INFRASTRUCTURE.  A draw is excused (sampler_cases.Ref.excused) when u lies
within 1e-6 of a step of the reference's CDF: delta = 0, because the kept set is exact for min-p and, by MARGIN, unambiguous for Mirostat."""
import functools
import math
from dataclasses import dataclass

import numpy as np

import nucleus_cases as nc
from nucleus_cases import MAX_EXCUSED, US, V, Ref, counts_of, logits_of, splitmix_u  # noqa: F401  (shared with the tests)

LN2, MU_STEPS, MARGIN = 0.693147180559945309417232121458, 64, 1e-9      # a Mirostat run follows mu over the first 64 of the 66 draws


@dataclass(frozen=True)
class Run:
    kind: str                    # "minp" | "mirostat"
    temp: float
    par: float                   # min_p | tau
    eta: float = 0.0
    mu0: float = None            # Mirostat: mu in front of the first draw (None: 2 tau, as the loops start)
    ban0: bool = False
    presence: float = 0.0
    frequency: float = 0.0

    def kw(self):          # the keywords of RWKV.sample_floor
        own = dict(min_p=self.par) if self.kind == "minp" else dict(tau=self.par, eta=self.eta)
        return dict(temp=self.temp, presence=self.presence, frequency=self.frequency, **own)


def reference(logits, run, counts=None, mu=None, ban0=None):      # (Ref, S): the draw of one row, and every token's surprise (None for min-p)
    l = nc.penalised(logits, counts, run.presence, run.frequency, run.ban0 if ban0 is None else ban0)
    mx = l.max()
    t = float(np.float32(run.temp))
    lw = (l - mx) * (1.0 if t == 1.0 else 1.0 / t)
    S = None
    with np.errstate(invalid="ignore"):
        if run.kind == "minp":
            kept = l - mx >= math.log(float(np.float32(run.par)))
        else:
            S = (math.log(np.exp(lw[l > -np.inf]).sum()) - lw) / LN2
            kept = S <= mu if (S <= mu).any() else l == mx
    w = np.where(kept, np.exp(np.where(kept, lw, -np.inf)), 0.0)
    c = np.cumsum(w)
    nz = np.nonzero(w > 0)[0]
    return Ref(w=w, c=c, steps=c[nz[:-1]] / c[-1], eps=nc.EPS, last=int(nz[-1])), S


def mu_next(run, S, pick, mu):
    return mu - float(np.float32(run.eta)) * (S[pick] - float(np.float32(run.par)))


@functools.lru_cache(maxsize=None)
def draws_of(lname, run, counted=False, shift=0):      # [(u, Ref, pick, mu before, mu after, margin = min |S_i - mu| / max(1, mu))], computed once
    lg, cnt = logits_of(lname, run.ban0), counts_of(lname, shift) if counted else None
    if run.kind == "minp":
        r, _ = reference(lg, run, cnt)
        return [(u, r, r.pick(u), None, None, None) for u in US]
    out, mu = [], 2.0 * float(np.float32(run.par)) if run.mu0 is None else run.mu0
    for u in US[:MU_STEPS]:
        r, S = reference(lg, run, cnt, mu)
        g, fin = r.pick(u), np.isfinite(S)
        out.append((u, r, g, mu, mu_next(run, S, g, mu), float(np.abs(S[fin] - mu).min()) / max(1.0, mu)))
        mu = out[-1][4]
    return out


# ---- the runs: (label, logits name, run, counted, count rotation, logits row, slot).  The min-p grid on case a, plain and with penalties and the ban; the other
# planted cases at the extremes; the Mirostat grid and one run that starts in the fallback; rows 0, 1, 2 with another slot (blockIdx.y, the 4 r bytes of row r)
MINP_GRID = tuple((t, p) for p in (1.0, 0.5, 0.05, 1e-6) for t in (0.003, 1.0, 1.5))
_EDGE = ((1.0, 1.0), (1.5, 0.05), (0.003, 1e-6))
# (min_p 1e-6 at temp 1 runs on case c, not a or b: their 8355 / 50277 kept tokens put 4 of the 66 draws within 1e-6 of a step)
RUNS = ([("c" if (t, p) == (1.0, 1e-6) else "a",) * 2 + (Run("minp", t, p), False, 0, 0, 0) for (t, p) in MINP_GRID] +
        [("p", "a", Run("minp", t, p, ban0=True, presence=0.4, frequency=0.4), True, 0, 0, 0) for (t, p) in MINP_GRID] +
        [(n, n, Run("minp", t, p, ban0=ban), False, 0, 0, 0) for n in ("c", "d2", "d50", "d1025", "e") for ban in (False, True) for (t, p) in _EDGE] +
        [("f", "f", Run("minp", 1.0, 0.05, ban0=True), False, 0, 0, 0), ("b", "b", Run("minp", 1.5, 0.05), False, 0, 0, 0), ("b", "b", Run("minp", 1.0, 0.5), False, 0, 0, 0)] +
        [("a", "a", Run("mirostat", t, tau, eta), False, 0, 0, 0) for tau in (0.5, 3.0, 8.0) for eta in (0.1, 1.0) for t in (0.7, 1.0)] +
        [(n, n, Run("mirostat", 1.0, 3.0, 0.1), False, 0, 0, 0) for n in ("b", "c", "d50", "e")] +
        [("c", "c", Run("mirostat", 0.7, 3.0, 0.1, mu0=0.25), False, 0, 0, 0)] +
        [(f"r/{n}", n, r, r.kind == "minp", slot, row, slot) for (n, row, slot) in (("a", 0, 2), ("c", 1, 0), ("d50", 2, 1))
         for r in (Run("minp", 1.0, 0.05, presence=0.4, frequency=0.4), Run("mirostat", 0.7, 3.0, 1.0, ban0=True))])
IDS = [f"{x[0]}-{r.kind}-t{r.temp}-{r.par}-eta{r.eta}-mu{r.mu0}-{'ban0' if r.ban0 else 'noban'}-pen{r.presence}" for x in RUNS for r in [x[2]]]
