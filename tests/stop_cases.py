"""Stop sequences and budgets (include/rwkv_mi355x.h rwkv_decode_batch_until): the Python restatement of the scan the device makes
behind every pick (csrc/stop.hip.h k_stop_step; include/rwkv_sampler.h stop_scan is its C++ twin), and the planted id strings the CPU
and GPU suites run it over.  Every comparison made with these is exact."""
import numpy as np

VOCAB = 50277
MAX_SEQS, MAX_LEN, POLL = 16, 8, 8
STEPS = 24
A, B, C_, D, Z = 11, 22, 33, 44, 7          # four symbols and a filler that no stop sequence holds
LO, HI = 1, VOCAB - 1                       # the smallest and the largest id a stream can produce


def stop_scan(ids, first, stops, max_new=None, history=None):
    """(len, reason, history) of ONE stream: ids = its picks g_0 .. g_{n-1} after `first`; stops = lists of ids; max_new = its budget
    (None or n: none); history = the newest ids of the previous call, oldest first (None: start with `first`; it continues only if it
    ends in `first`).  len counts the ids up to and including the one that stopped the stream; reason 0 ran all n, 1 budget, 2 + j
    sequence j (the lowest j of several, a sequence before the budget).  The returned history holds the newest 7 ids scanned."""
    h = [int(v) for v in history] if history is not None else []
    if not h or h[-1] != int(first):
        h = [int(first)]
    n = len(ids)
    for k, g in enumerate(ids):
        h.append(int(g))
        reason = 0
        for j, q in enumerate(stops):
            if len(q) <= len(h) and h[-len(q):] == [int(v) for v in q]:
                reason = 2 + j
                break
        if not reason and max_new is not None and k + 1 == max_new and k + 1 < n:
            reason = 1
        h = h[-(MAX_LEN - 1):]
        if reason:
            return k + 1, reason, h
    return n, 0, h


def scan_all(ids, firsts, stops, max_new=None):
    """(len [n], reason [n]) of the restatement over planted ids [n][steps]"""
    out = [stop_scan(ids[s], firsts[s], stops, None if max_new is None else max_new[s])[:2] for s in range(len(ids))]
    return np.array([o[0] for o in out], np.int64), np.array([o[1] for o in out], np.int64)


def bound(lmax, n_steps):
    """the largest steps_run of a call whose longest stream has lmax tokens"""
    return min(n_steps, POLL * ((lmax - 1) // POLL + 2))


def pad(head, steps=STEPS, fill=Z):
    head = list(head)
    return head + [fill] * (steps - len(head))


def _eight(k):
    return [A, B, C_, D, B, A, D, C_][:k]


# One planted call = the stop sequences it passes, and per stream (first token, the 24 picks, the budget or None).
PLANTED = {
    "self_overlap": dict(stops=[[A, A]], streams=[
        (B, pad([A, A, A]), None),                  # a a a: stops at the second a, once
        (A, pad([A, A, A]), None),                  # the match begins in first_token
        (B, pad([A, B, A, B, A, A]), None)]),
    "suffix_of_another": dict(stops=[[A, B, C_], [B, C_]], streams=[
        (Z, pad([D, A, B, C_]), None),              # both end here: the lowest j wins
        (Z, pad([D, D, B, C_]), None),              # only the suffix
        (A, pad([B, C_]), None)]),                  # the longer one begins in first_token
    "suffix_listed_first": dict(stops=[[B, C_], [A, B, C_], [C_]], streams=[
        (Z, pad([D, A, B, C_]), None),
        (Z, pad([D, C_]), None)]),
    "last_step": dict(stops=[[A, B], [D]], streams=[
        (Z, pad([Z] * (STEPS - 2) + [A, B]), None),
        (Z, pad([Z] * (STEPS - 1) + [D]), None),
        (Z, pad([Z] * (STEPS - 1) + [A]), None)]),  # one short of a match: ran all
    "first_token": dict(stops=[[A, B], [A, B, C_, D]], streams=[
        (A, pad([B]), None),
        (B, pad([A]), None),                        # the wrong way round: nothing
        (A, pad([A, B]), None)]),
    "len_1_and_8": dict(stops=[_eight(8), [D]], streams=[
        (Z, pad([Z, Z] + _eight(8)), None),         # the 8-gram holds D at its fourth place: the single id wins earlier
        (Z, pad([D]), None),
        (Z, pad(_eight(3)), None)]),
    "len_8_alone": dict(stops=[_eight(8)], streams=[
        (Z, pad([Z, Z] + _eight(8)), None),
        (A, pad(_eight(8)[1:]), None),              # begins in first_token: 7 picks complete it
        (Z, pad(_eight(7) + [Z] + _eight(8)), None),
        (Z, pad(_eight(4) + _eight(8)), None)]),
    "ids_1_and_50276": dict(stops=[[LO], [HI, LO], [HI, HI]], streams=[
        (HI, pad([HI], fill=2), None),
        (LO, pad([2, 2, LO], fill=2), None),
        (2, pad([HI, LO], fill=2), None),
        (2, pad([2, HI, 2, HI, HI], fill=2), None)]),
    "budget_1": dict(stops=[[A, B]], streams=[
        (Z, pad([Z, A, B]), 1),
        (A, pad([B]), 1),                           # budget and sequence at the same step: the sequence wins
        (Z, pad([Z, A, B]), 3),                     # again at step 3
        (Z, pad([Z, A, B]), 2),
        (Z, pad([Z] * STEPS), STEPS),               # a budget of n_steps is no stop
        (Z, pad([Z] * STEPS), STEPS - 1)]),
    "budget_only": dict(stops=[], streams=[(Z, pad([A, B, C_]), 1 + s % 5) for s in range(7)]),
    "sixteen": dict(stops=[[100 + j] * (1 + j % MAX_LEN) for j in range(MAX_SEQS)], streams=[
        (Z, pad([Z] * (j + 1) + [100 + j] * (1 + j % MAX_LEN)), None) for j in range(MAX_SEQS)]),
}


def many_streams(n=96, seed=1, steps=STEPS):
    """n random streams over the four symbols, a few random stop sequences and budgets on every third stream: matches are frequent"""
    rng = np.random.default_rng(seed)
    sym = np.array([A, B, C_, D])
    ids = sym[rng.integers(0, 4, (n, steps))]
    firsts = sym[rng.integers(0, 4, n)]
    stops = [[int(v) for v in sym[rng.integers(0, 4, int(rng.integers(2, 6)))]] for _ in range(4)]
    max_new = [int(1 + rng.integers(0, steps)) if s % 3 == 0 else steps for s in range(n)]
    return ids, firsts, stops, max_new


def random_case(rng):
    """one random stream of 1 .. 24 picks over the four symbols, for the twin: (first, ids, stops, max_new or None, history or None)"""
    sym = [A, B, C_, D]
    n = int(rng.integers(1, STEPS + 1))
    ids = [sym[i] for i in rng.integers(0, 4, n)]
    first = sym[int(rng.integers(0, 4))]
    stops = [[sym[i] for i in rng.integers(0, 4, int(rng.integers(1, MAX_LEN + 1)))] for _ in range(int(rng.integers(0, 5)))]
    max_new = int(rng.integers(1, n + 1)) if rng.integers(0, 2) else None
    history = None
    if rng.integers(0, 2):
        history = [sym[i] for i in rng.integers(0, 4, int(rng.integers(1, MAX_LEN)))]
        if rng.integers(0, 4):
            history[-1] = first                     # mostly a history that continues
    return first, ids, stops, max_new, history


KEEP_SEQ = [A, B, C_, D]                            # the 4-token sequence of the split cases


def keep_streams():
    """(firsts, ids [4][24]): KEEP_SEQ planted so that a split at step 12 cuts it at every position (0 .. 3 of its ids in the first call)"""
    ids = [pad([Z] * (12 - cut) + KEEP_SEQ) for cut in range(4)]
    return [Z] * 4, np.array(ids, np.int64)
