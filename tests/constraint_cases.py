"""Automata, bias lists, planted logits rows and the numpy restatement of constrained decoding (include/rwkv_mi355x.h "constrained decoding"),
shared by tests/test_constraint_cpu.py (the host twins of include/rwkv_sampler.h) and tests/test_constraint_gpu.py (csrc/constrain.hip.h).

The numpy reference of a constrained row is np.where(mask, l + b, -inf) in f32: ONE f32 add per allowed id, b = 0 where an id is not listed.
Everything compared against it is compared bit for bit -- there is no tolerance anywhere in these suites: the constrained pick is the existing
pick on the same numbers."""
import os
import re

import numpy as np

from support import CSRC

V = 50277
WORDS = 1572                      # mask words per state


def kernel_constants():
    """CN_SLICES, CN_NT of csrc/constrain.hip.h: how k_constrain_rows splits a row"""
    src = open(os.path.join(CSRC, "constrain.hip.h")).read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % k, src).group(1)) for k in ("CN_SLICES", "CN_NT"))


def slice_bounds(row):
    """first ids of the slices of logits row `row` (row r starts 4 r bytes past a 16-byte boundary: h elements in front of the aligned body)"""
    slices, _ = kernel_constants()
    h = (4 - row % 4) % 4
    nv = (V - h) >> 2
    return [h + 4 * ((p * nv) // slices) for p in range(1, slices)] + [h, h + 4 * nv]


def boundary_ids():
    """every multiple of 1024 and every slice boundary of the four row alignments, each with its two neighbours: the ids that straddle a
    workgroup's slice, a mask word or the head / body / tail split of a row"""
    ids = set()
    for b in list(range(0, V + 1024, 1024)) + [x for r in range(4) for x in slice_bounds(r)]:
        ids.update((b - 1, b, b + 1))
    return sorted(i for i in ids if 1 <= i < V)


def csr(rows):
    """rows: per state a list of (tok, next) -> (row_ptr, tok, next) u32, tok ascending inside a row"""
    row_ptr, tok, nxt = [0], [], []
    for r in rows:
        for t, n in sorted(r):
            tok.append(t); nxt.append(n)
        row_ptr.append(len(tok))
    return np.array(row_ptr, np.uint32), np.array(tok, np.uint32), np.array(nxt, np.uint32)


# the automaton of the planted-row suites.  States 2 and 3 are ADJACENT rows with the same ids and different next; state 0 is a one-edge row
P_ONE, P_LAST, P_TRIPLE, P_TRIPLE2, P_TAIL, P_BOUND, P_ALL = range(7)
PLANTED_STATES = {"one": P_ONE, "last": P_LAST, "triple": P_TRIPLE, "tail": P_TAIL, "boundaries": P_BOUND, "everything": P_ALL}


def planted_automaton():
    return csr([
        [(1, 1)],
        [(V - 1, 2)],
        [(31, 3), (32, 4), (33, 5)],
        [(31, 6), (32, 0), (33, 1)],
        [(i, 0) for i in range(50272, V)],
        [(i, 6) for i in boundary_ids()],
        [(i, i % 6) for i in range(1, V)],
    ])


def allowed_mask(a, q):
    """bool [V]: the ids state q allows; a terminal state allows every id but 0 (the row a stream keeps running on behind its end)"""
    row_ptr, tok, _ = a
    m = np.zeros(V, bool)
    if row_ptr[q] == row_ptr[q + 1]:
        m[1:] = True
    else:
        m[tok[row_ptr[q]:row_ptr[q + 1]]] = True
    return m


def mask_words(m):
    """the device's bit mask of one state: u32 [1572], bit i of word i // 32 = id i; 27 padding bits stay 0"""
    bits = np.zeros(WORDS * 32, np.uint8)
    bits[:V] = m
    return np.packbits(bits.reshape(WORDS, 32), axis=1, bitorder="little").view("<u4").reshape(WORDS)


def bias_vector(bias):
    b = np.zeros(V, np.float32)
    for t, v in (bias or {}).items():
        b[int(t)] = np.float32(v)
    return b


def constrained(l, m, bias=None):
    """the numpy reference: c = where(mask, l + b, -inf) in f32"""
    with np.errstate(invalid="ignore"):
        return np.where(m, np.asarray(l, np.float32) + bias_vector(bias), np.float32(-np.inf)).astype(np.float32)


def next_state(a, q, g):
    row_ptr, tok, nxt = a
    for e in range(int(row_ptr[q]), int(row_ptr[q + 1])):
        if tok[e] == g:
            return int(nxt[e])
    return int(q)


def argmax_low(c):
    """ties to the lowest id; id 0 never (it is -inf in every constrained row)"""
    return int(np.argmax(c))


def planted_row(m, seed=0):
    """f32 [V]: random logits in which every masked id lies 50 or more above the best allowed one, so that a pick that ignored the mask shows;
    two allowed ids tie for the maximum when the set has two or more (ties go to the lowest id)"""
    rng = np.random.default_rng(1000 + seed)
    l = (rng.standard_normal(V) * 3).astype(np.float32)
    ids = np.flatnonzero(m)
    if len(ids) >= 2:
        hi = rng.choice(ids, 2, replace=False)
        l[hi] = np.float32(l[ids].max() + 1.5)
    best = l[ids].max()
    l[~m] = (best + 50 + rng.random(int((~m).sum())) * 4).astype(np.float32)
    l[rng.choice(ids, 1)] = np.float32(-0.0)          # l + 0 is +0.0: the one add shows in the bits
    return l


# ---- the automaton of the loop suites: 6 states, allowed sets of 3 .. 400 ids drawn with a fixed seed, one state allowing everything ----
def loop_automaton(seed=7, states=6):
    rng = np.random.default_rng(seed)
    rows = []
    for q in range(states - 1):
        size = int(rng.integers(3, 401)) if q else 3
        ids = rng.choice(np.arange(1, V), size, replace=False)
        rows.append([(int(i), int(rng.integers(0, states))) for i in ids])
    rows.append([(i, int((i * 7) % states)) for i in range(1, V)])
    return csr(rows)


def everything_automaton():
    """one state, 50276 self-loops"""
    return csr([[(i, 0) for i in range(1, V)]])


CHOICES = [[100, 200], [100, 201, 300], [100, 201, 301], [5000, 6000, 7000, 8000]]     # a shared prefix, lengths 2, 3, 3, 4


def trie_accepts(a, seq):
    """the sequence leads from state 0 to a state without edges"""
    row_ptr, tok, nxt = a
    q = 0
    for g in seq:
        e = [e for e in range(int(row_ptr[q]), int(row_ptr[q + 1])) if tok[e] == g]
        if not e:
            return False
        q = int(nxt[e[0]])
    return row_ptr[q] == row_ptr[q + 1]


# ---- malformed inputs, by the name constraint_check gives the rule (include/rwkv_sampler.h) ----
def malformed():
    """[(rule, kwargs of the pybind module's constraintCheck)]"""
    u, f = (lambda *v: np.array(v, np.uint32)), (lambda *v: np.array(v, np.float32))
    ok = dict(S=2, row_ptr=u(0, 2, 3), tok=u(5, 9, 7), next=u(1, 0, 1))
    many = np.arange(1, 302, dtype=np.uint32)
    return [
        ("row_ptr", dict(ok, row_ptr=u(0, 3, 2))),                       # non-monotone
        ("row_ptr", dict(ok, row_ptr=u(1, 2, 3))),                       # does not start at 0
        ("row_ptr_end", dict(ok, row_ptr=u(0, 1, 2))),                   # row_ptr[S] != nnz
        ("tok_order", dict(ok, tok=u(9, 5, 7))),                         # unsorted inside a row
        ("tok_order", dict(ok, tok=u(5, 5, 7))),                         # duplicate
        ("tok_range", dict(ok, tok=u(0, 9, 7))),                         # id 0
        ("tok_range", dict(ok, tok=u(5, V, 7))),                         # >= 50277
        ("next", dict(ok, next=u(1, 2, 1))),                             # next >= S
        ("states", dict(S=0, row_ptr=u(0), tok=u(), next=u())),
        ("states", dict(S=4097, row_ptr=np.zeros(4098, np.uint32), tok=u(), next=u())),
        ("bias_count", dict(bias_tok=many, bias_val=np.zeros(301, np.float32))),
        ("bias_value", dict(bias_tok=u(3, 4), bias_val=f(1.0, np.nan))),
        ("bias_value", dict(bias_tok=u(3, 4), bias_val=f(np.inf, 1.0))),
        ("bias_order", dict(bias_tok=u(4, 3), bias_val=f(1.0, 1.0))),
        ("bias_order", dict(bias_tok=u(4, 4), bias_val=f(1.0, 1.0))),
        ("bias_range", dict(bias_tok=u(0, 3), bias_val=f(1.0, 1.0))),
        ("bias_range", dict(bias_tok=u(3, V), bias_val=f(1.0, 1.0))),
    ]


def well_formed():
    u, f = (lambda *v: np.array(v, np.uint32)), (lambda *v: np.array(v, np.float32))
    rp, tk, nx = planted_automaton()
    return [
        dict(S=2, row_ptr=u(0, 2, 3), tok=u(5, 9, 7), next=u(1, 0, 1)),
        dict(S=1, row_ptr=u(0, 0), tok=u(), next=u()),                                       # one terminal state
        dict(S=len(rp) - 1, row_ptr=rp, tok=tk, next=nx),
        dict(S=4096, row_ptr=np.zeros(4097, np.uint32), tok=u(), next=u()),
        dict(bias_tok=np.arange(1, 301, dtype=np.uint32), bias_val=np.full(300, -np.inf, np.float32)),
        dict(bias_tok=u(1, V - 1), bias_val=f(-3.5, 1e30)),
        dict(bias_tok=u(), bias_val=f()),
    ]
