"""The ratio rule of speculative sampling (include/rwkv_mi355x.h rwkv_spec_ratio_rows) restated in plain f64 numpy, and the planted row pairs the
device pick is held to.  A DRAW is (l, m, x, Tt, Td, u_a, u_r); draws() asserts on the CPU that each one is decided with room -- log u_a at least
1e-6 from lp(x) - lq(x), u_r R at least 1e-9 R from the cumulative sum on either side of the chosen id -- so no draw needs excusing on the GPU.
TEST INFRASTRUCTURE: nothing here is imported by the product."""
import numpy as np

from sampler_cases import splitmix_u

V = 50277


def logp(row, temp):                          # lp(i) = (s_i - M) - log Z with s = row / temp, M and Z over the ids >= 1
    inv = 1.0 if np.float32(temp) == 1 else 1.0 / np.float64(np.float32(temp))
    s = np.asarray(row, np.float32).astype(np.float64) * inv
    M = s[1:].max()
    return (s - M) - np.log(np.exp(s[1:] - M).sum())


class Rule:
    """one row pair under the rule: delta = lp(x) - lq(x), the residual r, its cumulative sum in id order"""

    def __init__(self, l, m, x, Tt=1.0, Td=1.0):
        self.l, self.x = np.asarray(l, np.float32), x
        self.p = np.exp(logp(l, Tt))
        self.q = np.zeros(V) if x is None else np.exp(logp(m, Td))
        self.delta = None if x is None or x == 0 else logp(l, Tt)[x] - logp(m, Td)[x]
        self.p[0] = self.q[0] = 0.0
        self.r = np.maximum(self.p - self.q, 0.0)
        if x is not None:
            self.r[x] = 0.0
        self.cum = np.cumsum(self.r)
        self.R = self.cum[-1]

    def accepts(self, u_a):
        return self.delta is not None and (u_a == 0.0 or np.log(u_a) < self.delta)

    def pick(self, u_a, u_r):                 # (id, accepted)
        if self.accepts(u_a):
            return self.x, 1
        if self.R == 0.0:
            g = self.l.copy()
            g[[0] + ([] if self.x is None else [self.x])] = -np.inf
            return int(np.argmax(g)), 0
        return int(np.searchsorted(self.cum, u_r * self.R, side="right")), 0

    def decided(self, u_a, u_r):
        if self.delta is not None and u_a > 0.0 and abs(np.log(u_a) - self.delta) < 1e-6:
            return False
        if self.accepts(u_a) or self.R == 0.0:
            return True
        i, t = self.pick(u_a, u_r)[0], u_r * self.R
        return self.cum[i] - t >= 1e-9 * self.R and t - (self.cum[i - 1] if i else 0.0) >= 1e-9 * self.R

    def u_at(self, i):                        # the u_r in the middle of id i's step of the cumulative sum
        return float(((self.cum[i - 1] if i else 0.0) + 0.5 * self.r[i]) / self.R)


def _base(seed):
    return (np.random.default_rng(seed).standard_normal(V) * 2.0).astype(np.float32)


def _boosted(ids, boost=3.0, seed=1, x=7777, level=None):
    """m = a base row, l = the same with `ids` raised (so the residual lives exactly on ids) and x lowered (so x is rejected)"""
    m = _base(seed)
    if level is not None:
        m[ids] = level                        # equal logits under equal boosts: exact ties of r
    l = m.copy()
    l[ids] += np.float32(boost)
    l[x] -= np.float32(30.0)
    return l, m, x


# 50-id ownership of the samplers, the 64-id groups and the 3200-id waves of k_ratio_pick, the last wave and the last id
EDGES = [49, 50, 51, 63, 64, 65, 3199, 3200, 3201, 3263, 3264, 47999, 48000, 50239, 50240, V - 1]


def cases():
    """name -> (l, m, x, Tt, Td, ids to land on (None: a few by u alone), expected support of r or None)"""
    c = {}
    b = _base(2)
    c["equal"] = (b, b.copy(), 4321, 0.8, 0.8, None, [])                                     # q bitwise p: every u_a < 1 accepts
    m = _base(3); m[911] += 25.0
    c["q_peaked_on_x"] = (_base(3), m, 911, 1.0, 1.0, [1, 910, 912, 25000, V - 1], None)     # p(x) tiny against q(x): rejected, pick != x
    c["ends"] = _boosted([1, V - 1]) + (1.0, 1.0, [1, V - 1], [1, V - 1])
    c["edges"] = _boosted(EDGES) + (1.0, 1.0, EDGES, EDGES)
    c["ties"] = _boosted([63, 64, 3199, 3200, 3201], level=1.5) + (1.0, 1.0, [63, 64, 3199, 3200, 3201], [63, 64, 3199, 3200, 3201])
    l, m, x = _boosted([5, 40000])
    l[0] = m[0] = 60.0
    c["id0_largest"] = (l, m, x, 1.0, 1.0, [5, 40000], [5, 40000])
    hi = _base(4); hi[1234] = hi.max() + 800.0
    c["peak_p"] = (hi, _base(5), 99, 1.0, 1.0, [1234], [1234])
    c["peak_q"] = (_base(5), hi, 1234, 1.0, 1.0, [1, 1233, 1235, V - 1], None)
    hq = hi.copy(); hq[99] += 5.0
    c["peak_both"] = (hi, hq, 99, 1.0, 1.0, None, [])                                        # x rejected and R == 0: the greedy rule, id 1234
    c["peak_both_x"] = (hi, hi.copy(), 1234, 1.0, 1.0, None, [])                             # delta == 0: accepted
    c["bonus"] = (_base(6), None, None, 0.7, 1.0, [1, 50, 64, 3200, V - 1], None)
    c["bonus_peak"] = (hi, None, None, 1.0, 1.0, [1234], [1234])
    cold = _base(7); cold[[300, 40001]] = [12.0, 12.0 - 0.003]                                 # Tt = 0.003: two ids share the mass e : 1
    c["cold_target"] = (cold, _base(8), 5000, 0.003, 1.0, [300, 40001], None)
    c["cold_draft"] = (_base(8), cold, 300, 1.3, 0.003, [1, 299, 301, V - 1], None)          # q a point mass on x
    c["x_is_0"] = (_base(9), _base(10), 0, 1.0, 1.0, None, None)                             # an id neither side emits: rejected
    return c


def draws():
    """name -> list of (l, m, x, Tt, Td, u_a, u_r), every one decided with room"""
    out = {}
    for name, (l, m, x, Tt, Td, land, support) in cases().items():
        ru = Rule(l, m, x, Tt, Td)
        if support is not None:
            assert sorted(np.flatnonzero(ru.r)) == sorted(support), name
        u_rs = [ru.u_at(i) for i in land] if land else [1e-7, 0.37, 0.999999]
        u_as = [0.0, 0.5, 0.999]
        if ru.delta is not None and -700.0 < ru.delta < 0.0:                                 # one draw on either side of the ratio
            u_as += [float(np.exp(ru.delta) * 0.5), float(min(np.exp(ru.delta) * 2.0, 0.9999))]
        ds = [(l, m, x, Tt, Td, u_a, u_r) for u_a in u_as for u_r in u_rs if ru.decided(u_a, u_r)]
        assert len(ds) >= len(u_rs), name
        out[name] = ds
    out["mixed"] = [ds[i % len(ds)] for i, ds in enumerate(out.values())] * 3                # rows of different content in one call
    return out


def verify_ref(rows, q_rows, draft, Tt, Td, seed, step0):
    """(n_accepted, next, every row 0 .. a decided with room) of rwkv_spec_verify_ratio from the downloaded logits rows [n_draft + 1][V]"""
    ok = True
    for j, x in enumerate(list(draft) + [None]):                       # (the bonus row never accepts: the loop returns)
        ru = Rule(rows[j], None if x is None else q_rows[j], x, Tt, Td)
        u_a, u_r = splitmix_u(seed, 2 * (step0 + j)), splitmix_u(seed, 2 * (step0 + j) + 1)
        ok, (t, acc) = ok and ru.decided(u_a, u_r), ru.pick(u_a, u_r)
        if not acc:
            return j, t, ok
