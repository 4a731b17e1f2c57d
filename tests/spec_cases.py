"""Speculative greedy decoding (include/rwkv_mi355x.h rwkv_spec_verify / rwkv_decode_speculative): the cases of tests/test_spec_cpu.py and
tests/test_spec_gpu.py, and a pure-Python STATEMENT of the pick, of accept / commit and of the round loop over any `forward(rows, state)` -- run on
the CPU oracle by the CPU suite, compared with the device by the GPU suite.

The models are modelfile.synthetic_tensors, three layers deep, every context loaded with max_ctx = 34.  Widths: 64 (the smallest chunk width:
octants of 8 channels, WKV workgroups partly filled), 320 (no power of two, uneven octants), 1024, and one 4096-wide two-layer case."""

import numpy as np

V = 50277
MAXT = 34
MAX_DRAFT = 31
WIDTHS = [(3, 64), (3, 320), (3, 1024), (2, 4096)]            # (layers, width)
SEED = 7300                                                    # + width: the models of the width cases
N_DRAFTS = (1, 2, 7, 31)
# test 5 (against plain decode) and the margin condition the CPU suite proves on the oracle alone: model, first token, tokens
PLAIN = dict(L=3, D=64, seed=7413, prompt=(5, 6, 7), first=101, n=48)      # (the prompt is fed from the zero state)
MARGIN = 1e-3                                                  # top-two gap over the row's largest |logit|, at every step of the continuation


def pick(row):
    """the greedy pick of a logits row as the device takes it: logit 0 banned, ties to the lowest id, no winner (nothing above -inf, NaN) -> 0"""
    l = np.array(row, np.float32, copy=True)
    l[0] = -np.inf
    l[np.isnan(l)] = -np.inf
    i = int(np.argmax(l))                                       # the first of equal maxima
    return i if l[i] > -np.inf else 0


def accept(draft, picks):
    """a = the number of leading i with draft[i] == picks[i]; picks has len(draft) + 1 entries"""
    a = 0
    while a < len(draft) and int(draft[a]) == int(picks[a]):
        a += 1
    return a


def verify(forward, state, token, draft):
    """the statement of rwkv_spec_verify over forward(rows, state) -> logits [len(rows)][V] (which advances `state`, a list of arrays, in place):
    every row is picked from a pass that commits nothing, and the state becomes the one after rows 0 .. a.  Returns (a, next, picks)."""
    rows = [int(token)] + [int(t) for t in draft]
    assert len(draft) <= MAX_DRAFT
    scratch = [s.copy() for s in state]
    picks = [pick(r) for r in forward(rows, scratch)]
    a = accept(draft, picks)
    forward(rows[:a + 1], state)                                # the commit of exactly row a
    return a, picks[a], picks


def loop(verify_fn, draft_fn, first, n_tokens, k):
    """the statement of the round loop: draft_fn(history, kd) guesses at most kd ids behind `history` (whose last id has not been fed),
    verify_fn(token, draft) -> (a, next).  Returns (ids, stats); never emits or consumes more than n_tokens."""
    out, hist = [], [int(first)]
    stats = dict(rounds=0, drafted=0, accepted=0)
    while len(out) < n_tokens:
        kd = min(k, n_tokens - len(out) - 1)
        d = [int(t) for t in draft_fn(hist, kd)][:kd] if kd > 0 else []
        a, nx = verify_fn(hist[-1], d)[:2]
        new = d[:a] + [int(nx)]
        out += new; hist += new
        stats["rounds"] += 1; stats["drafted"] += len(d); stats["accepted"] += a
    assert len(out) <= n_tokens
    return out, stats


def greedy(forward, state, first, n):
    """n greedy ids, one row at a time"""
    out, t = [], int(first)
    for _ in range(n):
        t = pick(forward([t], state)[0])
        out.append(t)
    return out


def gaps(forward, state, first, n):
    """(ids, gap / max |logit| per step) of the greedy continuation: the margin condition of test 5"""
    out, g, t = [], [], int(first)
    for _ in range(n):
        l = np.array(forward([t], state)[0], np.float64)
        l[0] = -np.inf
        top = np.sort(l)[-2:]
        g.append(float(top[1] - top[0]) / float(np.abs(l[1:]).max()))
        t = pick(l)
        out.append(t)
    return out, g


def wrong(t):
    """an id of the vocabulary other than t, and not 0"""
    return int(t) + 1 if int(t) + 1 < V else 1


def planted(g, n_draft):
    """the drafts of test 1 for one n_draft: (label, draft, a) with g's first n_draft ids and one wrong id at p in {0, middle, last, none}"""
    cases = []
    for label, p in (("first", 0), ("middle", n_draft // 2), ("last", n_draft - 1), ("none", None)):
        d = [int(t) for t in g[:n_draft]]
        if p is not None:
            d[p] = wrong(d[p])
        if (p, d) not in [(c[3], c[1]) for c in cases]:
            cases.append((label, d, n_draft if p is None else p, p))
    return [c[:3] for c in cases]


def edge_tensors(L, D, seed):
    """a model whose every row picks id 50276: ln_out's weight 0 and bias 1 make the head's input the constant 1, and the head's column 50276 is 255
    in every row of the matrix where no other column is"""
    from rwkv_cpp_accelerated_amd import modelfile as mf
    t = mf.synthetic_tensors(L, D, seed=seed)
    ln = t[mf.LAYERNORMS].reshape(4 * (L + 1), D).copy()
    ln[4 * L + 2] = 0.0
    ln[4 * L + 3] = 1.0
    t[mf.LAYERNORMS] = ln.reshape(-1)
    h = t[mf.HEAD].reshape(D, V).copy()
    h[:, V - 1] = 255
    h[0, : V - 1] = np.minimum(h[0, : V - 1], 254)
    t[mf.HEAD] = h.reshape(-1)
    return t
