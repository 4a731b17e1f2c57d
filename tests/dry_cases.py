"""DRY penalties (include/rwkv_mi355x.h rwkv_decode_batch_dry): the plain Python / numpy restatement of the scan and of the penalty, and the planted
histories on which csrc/dry.hip.h k_dry_scan and include/rwkv_sampler.h dry_scan are held to it.  TEST INFRASTRUCTURE: no product code imports it."""
import numpy as np

V = 50277
MAX_WINDOW, MAX_MATCH = 4096, 64


def scan(history, allowed_length=2, window=MAX_WINDOW, breakers=()):
    """[(id, L)] ascending by id: the header's definition, word for word"""
    h = [int(t) for t in history][-window:]
    n, best = len(h), {}
    if n < 2 or h[-1] in breakers:
        return []
    for j in range(n - 1):
        if h[j] != h[-1]:
            continue
        m = 0
        while m < MAX_MATCH and j - m >= 0 and h[j - m] == h[n - 1 - m] and h[j - m] not in breakers:
            m += 1
        best[h[j + 1]] = max(best.get(h[j + 1], 0), m)
    return sorted((t, l) for t, l in best.items() if l >= allowed_length)


def table(multiplier, base):
    """pen[i] f32: p_0 = multiplier, p_(i+1) = p_i * base in f64, each rounded once"""
    pen, p = np.zeros(MAX_MATCH, np.float32), float(np.float32(multiplier))
    with np.errstate(over="ignore"):
        for i in range(MAX_MATCH):
            pen[i] = np.float32(p)
            p *= float(np.float32(base))
    return pen


def penalised(c, history, multiplier, base, allowed_length=2, window=MAX_WINDOW, breakers=()):
    """the constrained row c (f32 [V]) behind the penalty: one f32 subtraction per penalised id"""
    out, pen = np.array(c, np.float32), table(multiplier, base)
    with np.errstate(invalid="ignore"):
        for t, l in scan(history, allowed_length, window, breakers):
            out[t] = np.float32(out[t]) - pen[l - allowed_length]
    return out


def _repeat(m, follower=50, pre=(11, 12)):
    """a run of m distinct ids, then `follower`, then the run again behind a different id: one hit of length exactly m (the cap aside)"""
    run = list(range(100, 100 + m))
    return [pre[0]] + run + [follower, pre[1]] + run


_R = np.random.default_rng(11)
_ALT = [x for f in range(20000, 20000 + 2047) for x in (7, f)] + [7, 7]      # 7 f 7 f' .. 7 7: every second start hits, 2048 distinct followers --
                                                                              # the most a window can hold, as a follower that is a start is `last`
# name -> (history, keywords of scan)
CASES = {
    "empty": ([], {}),
    "one_id": ([5], dict(allowed_length=1)),
    "two_ids": ([5, 5], dict(allowed_length=1)),
    "exactly_window": ([3] + _repeat(6), dict(window=16)),                    # 16 ids
    "window_plus_one": ([3, 3] + _repeat(6), dict(window=16)),
    "ring_wraps_4097": ([int(t) for t in _R.integers(1, 40, 4097)], dict(allowed_length=1)),
    "match_runs_into_the_window_start": ([1, 2, 3, 4, 50, 9, 1, 2, 3, 4], dict(window=8, allowed_length=1)),      # window: 3 4 50 9 1 2 3 4 -> L = 2, not 4
    "overlaps_the_tail_200": ([7] * 200, dict(allowed_length=1)),
    "one_id_fills_the_window": ([7] * 4096, {}),                              # 4095 hits on one key, every one at the cap
    "match_63": (_repeat(63), dict(allowed_length=63)),
    "match_64": (_repeat(64), dict(allowed_length=64)),
    "match_65": (_repeat(65), dict(allowed_length=64)),                              # capped
    "breaker_inside_a_match": (_repeat(10), dict(breakers=(104,), allowed_length=1)),      # L = 5: ids 105 .. 109
    "last_id_is_a_breaker": (_repeat(10), dict(breakers=(109,), allowed_length=1)),
    "one_follower_from_three_starts": ([1, 2, 3, 60, 8, 2, 3, 60, 9, 3, 60, 5, 1, 2, 3], dict(allowed_length=1)),   # L = 3, 2, 1: the max wins
    "allowed_minus_one": ([1, 2, 3, 60, 8, 2, 3, 61, 5, 1, 2, 3], dict(allowed_length=3)),                           # 60 at L = 3 stays, 61 at L = 2 goes
    "match_63_under_64": (_repeat(63), dict(allowed_length=64)),                                                     # allowed - 1 at the cap: nothing
    "followers_1_and_50276": ([4, 1, 4, V - 1, 4], dict(allowed_length=1)),
    "one_bucket": ([4, 3, 4, 8195, 4, 16387, 4, 3 + 5 * 8192, 4], dict(allowed_length=1)),    # ids 8192 apart: linear probing
    "most_followers": (_ALT, dict(allowed_length=1)),
}
# the answers that can be written out by hand: what holds the restatement itself
WANT = {"empty": [], "one_id": [], "two_ids": [(5, 1)], "exactly_window": [(50, 6)], "window_plus_one": [(50, 6)], "last_id_is_a_breaker": [],
        "match_runs_into_the_window_start": [(50, 2)], "overlaps_the_tail_200": [(7, 64)], "one_id_fills_the_window": [(7, 64)], "match_63": [(50, 63)],
        "match_64": [(50, 64)], "match_65": [(50, 64)], "match_63_under_64": [], "breaker_inside_a_match": [(50, 5)], "allowed_minus_one": [(60, 3)],
        "one_follower_from_three_starts": [(60, 3)], "followers_1_and_50276": [(1, 1), (V - 1, 1)]}


def expected(name):
    """the restatement's answer for a planted case (checked against the written-out one where there is one)"""
    want = scan(CASES[name][0], **CASES[name][1])
    assert WANT.get(name, want) == want, name
    return want
