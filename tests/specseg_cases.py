"""Speculative greedy decoding for many streams (include/rwkv_mi355x.h rwkv_spec_verify_segments): the cases of tests/test_specseg_cpu.py and
tests/test_specseg_gpu.py.  The models are modelfile.synthetic_tensors, every context loaded with max_ctx = 80 and started from
segment_cases.start_state (a history on all 80 slots).  Widths: 64 (the smallest), 320 (off the 256 grid) and the 7B width with two layers."""
import numpy as np

import spec_cases as sc

V, MAXT = sc.V, 80
WIDTHS = [(3, 64), (3, 320), (2, 4096)]                        # (layers, width)
SEED = 9100                                                    # + width: the models
MARGIN = 1e-3                                                  # top-two gap over the row's largest |logit|: 30 times the chunk path's logits bound
PROMPT = [7, 50000, 11, 9]                                     # what segment_cases.start_state feeds slot 0 behind the history

# layouts as (slot, n, n_draft, index of the first wrong draft id or None)
FIVE = [(5, 4, 3, 1), (0, 8, 7, None), (9, 2, 1, 0), (12, 5, 0, None), (3, 6, 2, 1)]
EIGHTS = [(s, 8, 7, w) for s, w in ((1, 2), (2, None), (4, 0), (6, 5), (8, 6), (10, None), (11, 3))]
LAYOUTS = dict(
    ONE_0=[(0, 8, 7, 0)], ONE_3=[(0, 8, 7, 3)], ONE_ALL=[(0, 8, 7, None)],     # also held to rwkv_spec_verify
    FIVE=FIVE, FIVE_REV=FIVE[::-1],
    R33=[(13, 1, 0, None)] + EIGHTS[:4],                       # rows 25 .. 32 are one segment: the first half is full, the second holds one row
    R64=[(13, 4, 3, None)] + EIGHTS + [(14, 4, 1, 0)],         # rows 28 .. 35 are one segment; the TCAP = 64 kernel with every row in use
    LONG=[(7, 32, 31, None)],
)


def certain(slot, n):
    """the n certain ids of the segment on `slot`: seeded, in 1 .. V - 1"""
    return [int(t) for t in np.random.default_rng(100 * slot + n).integers(1, V, n)]


def plant(layout, g):
    """g[i]: the n_draft + 1 greedy ids behind segment i's certain ids.  Returns (segments [(slot, ids, n_draft)] whose drafts are g with the
    layout's wrong id planted by spec_cases.wrong, the expected [(a, next, row)])"""
    segs, want, r0 = [], [], 0
    for (slot, n, nd, w), gi in zip(layout, g):
        d = list(gi[:nd])
        if w is not None:
            d[w] = sc.wrong(d[w])
        a = nd if w is None else w
        segs.append((slot, certain(slot, n - nd) + d, nd))
        want.append((a, gi[a], r0 + n - nd - 1 + a))
        r0 += n
    return segs, want


def gap(row):
    """top-two gap of a logits row (logit 0 banned) over its largest |logit|"""
    l = np.array(row, np.float64)
    l[0] = -np.inf
    top = np.partition(l, -2)[-2:]
    return float(top[1] - top[0]) / float(np.abs(l[1:]).max())


def oracle_verify(forward, st, ids, n_draft):
    """the statement of one segment over the oracle's forward(rows, state), which advances `st` in place: (a, next, the logits row `next` was
    picked from, the smallest gap of the rows that were picked)"""
    c = len(ids) - n_draft
    l, a = forward(ids[:c], st)[-1], 0
    g = [gap(l)]
    while a < n_draft and ids[c + a] == sc.pick(l):
        l = forward([ids[c + a]], st)[0]
        a += 1
        g.append(gap(l))
    return a, sc.pick(l), l, min(g)
