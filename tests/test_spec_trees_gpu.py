"""Draft trees for many streams on the device (include/rwkv_mi355x.h rwkv_spec_verify_trees, csrc/specseg.hip.h).  The greedy continuation of
every segment is built with rwkv_forward_segments alone, one id at a time; what a tree verify leaves -- records, accepted ids, slot state, the
logits rows of the certain rows and of the path -- is held bit for bit to rwkv_forward_segments of the certain and accepted ids, alone, from the
same start; a chain is held bit for bit to rwkv_spec_verify_segments.  One case is held to the f64 oracle within the chunk suite's bounds.
Every context has max_ctx = 80 and a history on all 80 slots."""
import ctypes as C

import numpy as np
import pytest

from rwkv_cpp_accelerated_amd import modelfile as mf
import parity
import segment_cases as sg
import spec_cases as sc
import specseg_cases as cs
import spectree_cases as tc
from support import E_ARG, NAMES, GuardContexts, check_refused, eng, load, restore, rows, same_state, snapshot  # noqa: F401

pytestmark = pytest.mark.gpu
V, MAXT = cs.V, cs.MAXT
WIDTHS = cs.WIDTHS[:2]


class Model:
    """one model with its start state and the greedy continuations asked of it (once per module)"""

    def __init__(self, eng, L, D):
        self.t = mf.synthetic_tensors(L, D, seed=cs.SEED + D)
        self.m = load(eng, L, D, 0, MAXT, self.t)
        sg.start_state(eng, self.m, D)
        self.start, self.g = snapshot(self.m, MAXT), {}

    def alone(self, slot, ids):
        """(state, logits rows) that rwkv_forward_segments of one segment leaves from the start state"""
        restore(self.m, self.start)
        self.m.forward_segments([(slot, ids)])
        return snapshot(self.m, MAXT), rows(self.m, len(ids))

    def greedy(self, heads, depth):
        """per (slot, certain ids) of `heads` the `depth` greedy ids behind them: step j feeds every head its certain ids and its first j greedy ids"""
        key = (tuple((s, tuple(ids)) for s, ids in heads), depth)
        if key not in self.g:
            g = [[] for _ in heads]
            for _ in range(depth):
                restore(self.m, self.start)
                last = self.m.forward_segments([(s, list(ids) + gi) for (s, ids), gi in zip(heads, g)])
                lg = self.m.logits(last[-1] + 1).reshape(-1, V)
                for gi, r in zip(g, last):
                    gi.append(sc.pick(lg[r]))
            self.g[key] = g
        return self.g[key]

    def planted(self, pass_rows, rot):
        heads = [(s, cs.certain(s, nc)) for s, nc in tc.HEADS[pass_rows]]
        g = self.greedy(heads, tc.DEPTH)
        behind_wrong = self.greedy([(s, ids + [sc.wrong(gi[0])]) for (s, ids), gi in zip(heads, g)], 1)      # the pick of node 0's row: the decoy's id
        return tc.planted(tc.HEADS[pass_rows], g, rot, [d[0] for d in behind_wrong])

    def verify(self, segs, call=None):
        """(records, state, logits rows) of a tree call from the start state"""
        restore(self.m, self.start)
        got = (call or self.m.spec_verify_trees)(segs)
        return got, snapshot(self.m, MAXT), rows(self.m, sum(len(s[1]) for s in segs))


@pytest.fixture(scope="module")
def models(eng):
    cache = {}

    def get(L, D):
        if (L, D) not in cache:
            cache[(L, D)] = Model(eng, L, D)
        return cache[(L, D)]
    yield get
    for w in cache.values():
        w.m.close()


@pytest.mark.parametrize("name", list(cs.LAYOUTS))
@pytest.mark.parametrize("L,D", WIDTHS)
def test_a_chain_is_the_segmented_verify(eng, models, L, D, name):
    """rwkv_spec_verify_segments and rwkv_spec_verify_trees on a chain are two entry points over ONE path (the chain call passes no parents and plans
    from[t] = t - 1 itself): this holds the host plumbing of both to each other.  The path's independent anchors: tests/test_specseg_gpu.py holds the
    verify bit for bit to rwkv_forward_segments alone and to rwkv_spec_verify, and to the f64 oracle; test_planted_trees and
    test_against_the_statement_over_the_oracle cover the trees."""
    w, lay = models(L, D), cs.LAYOUTS[name]
    g = w.greedy([(slot, cs.certain(slot, n - nd)) for slot, n, nd, _ in lay], 1 + max(nd for _, _, nd, _ in lay))
    segs, want = cs.plant(lay, [gi[:nd + 1] for gi, (_, _, nd, _) in zip(g, lay)])
    restore(w.m, w.start)
    assert w.m.spec_verify_segments(segs) == want, name
    state, lg = snapshot(w.m, MAXT), rows(w.m, sum(len(ids) for _, ids, _ in segs))
    got, state_t, lg_t = w.verify([s + (None,) for s in segs])
    assert [r[:3] for r in got] == want and [r[3] for r in got] == [ids[len(ids) - nd:len(ids) - nd + a] for (_, ids, nd), (a, _, _) in zip(segs, want)], name
    same_state(state_t, state, f"D{D} {name}")
    assert np.array_equal(lg_t, lg), f"D{D} {name}: logits rows"


def held_to_alone(w, segs, paths, got, state, lg, what, next_of=None):
    """every segment's record, slot and the logits rows of its certain rows and its path against rwkv_forward_segments of those ids, alone;
    `next` against the greedy pick of its last row, or against next_of(segment, slot, rows fed, a)"""
    r0 = 0
    for i, ((slot, ids, nd, _), path, (a, nx, row, em)) in enumerate(zip(segs, paths, got)):
        keep = list(range(len(ids) - nd)) + path
        assert (a, row, em) == (len(path), r0 + keep[-1], [ids[r] for r in path]), f"{what} slot {slot}"
        alone, alone_rows = w.alone(slot, [ids[r] for r in keep])
        assert nx == (next_of(i, slot, len(keep), a) if next_of else sc.pick(alone_rows[-1].view(np.float32))), f"{what} slot {slot}: next"
        for k, name in enumerate(NAMES):
            assert np.array_equal(state[k][slot], alone[k][slot]), f"{what} slot {slot}: {name}"
        assert np.array_equal(lg[[r0 + r for r in keep]], alone_rows), f"{what} slot {slot}: logits rows"
        r0 += len(ids)


@pytest.mark.parametrize("rot", range(3))
@pytest.mark.parametrize("pass_rows", [32, 64])
@pytest.mark.parametrize("L,D", WIDTHS)
def test_planted_trees(eng, models, L, D, pass_rows, rot):
    w = models(L, D)
    segs, paths = w.planted(pass_rows, rot)
    got, state, lg = w.verify(segs)
    what = f"D{D} {pass_rows} rows, kinds from {rot}"
    same_state(state, w.start, what + ", slots not named", [s for s in range(MAXT) if s not in [x[0] for x in segs]])
    assert np.array_equal(state[3], w.start[3]), what + ": pp"
    held_to_alone(w, segs, paths, got, state, lg, what)


@pytest.mark.parametrize("L,D", WIDTHS)
def test_every_segment_of_a_mixed_call_equals_itself_alone(eng, models, L, D):
    w = models(L, D)
    heads = [(5, cs.certain(5, 1)), (9, cs.certain(9, 2)), (0, cs.certain(0, 4))]
    g = w.greedy(heads, tc.DEPTH)
    trees = [tc.segment(s, len(ids), gi, kind)[0] for (s, ids), gi, kind in zip(heads, g, ("whole", "inner", "none"))]
    segs = trees[:2] + [(12, cs.certain(12, 5), 0, None), trees[2]]           # two trees, a plain segment, a prompt's tail followed by a tree: 36 rows
    got, state, lg = w.verify(segs)
    r0 = 0
    for seg, (a, nx, row, em) in zip(segs, got):
        ((a1, nx1, row1, em1),), state1, lg1 = w.verify([seg])
        assert (a, nx, row - r0, em) == (a1, nx1, row1, em1), f"D{D} slot {seg[0]}"
        for k, name in enumerate(NAMES):
            assert np.array_equal(state[k][seg[0]], state1[k][seg[0]]), f"D{D} slot {seg[0]}: {name}"
        assert np.array_equal(lg[r0:r0 + len(seg[1])], lg1), f"D{D} slot {seg[0]}: logits rows"
        r0 += len(seg[1])


def test_against_the_statement_over_the_oracle(eng, oracle, models):
    L, D = WIDTHS[0]
    w = models(L, D)
    segs, paths = w.planted(32, 0)
    got, state, lg = w.verify(segs)
    om = oracle.from_tensors(L, D, w.t)
    for (slot, ids, nd, _), path, (a, nx, row, em) in zip(segs, paths, got):
        st = [s.view(np.float64)[slot].copy() for s in w.start]
        a_ref, nx_ref, l_ref, gmin = cs.oracle_verify(om.forward, st, ids[:len(ids) - nd] + [ids[r] for r in path] + [0], len(path) + 1)
        what = f"D{D} slot {slot}"
        print(f"{what}: a {a} next {nx}, oracle a {a_ref} next {nx_ref}, smallest top-two gap {gmin:.2e}")
        assert gmin >= cs.MARGIN, what                                # (tests/test_spec_trees_cpu.py proves it on the oracle alone)
        assert (a, nx, em) == (a_ref, nx_ref, [ids[r] for r in path]), what
        for l in range(L):
            lo = slice(l * D, (l + 1) * D)
            for k, tol in ((0, parity.TOL), (1, 1e-4), (2, 1e-4), (4, parity.TOL)):
                parity._close(state[k].view(np.float64)[slot][lo], st[k][lo], f"{what} layer {l} {NAMES[k]}", tol)
        parity._close(lg[row].view(np.float32), l_ref, what + " committed row", parity.TOL)     # 3e-5 of the row's largest |logit|
    om.close()


@pytest.mark.parametrize("kind", ["greedy", "nucleus"])
@pytest.mark.parametrize("L,D", WIDTHS)
def test_sampled_acceptance(eng, models, L, D, kind):
    w, m = models(L, D), models(L, D).m
    segs, _ = w.planted(64, 1)
    seeds, step0 = [11 + i for i in range(len(segs))], [3 * i for i in range(len(segs))]
    picks = [eng.pick_of("greedy") if kind == "greedy" else eng.pick_of(temp=0.4, top_p=0.6)] * len(segs)
    got, state, lg = w.verify(segs, lambda s: m.spec_sample_trees(s, picks, seeds, step0))
    if kind == "greedy":                                              # RWKV_PICK_GREEDY: the tree verify itself
        got_v, state_v, lg_v = w.verify(segs)
        assert got == got_v and np.array_equal(lg, lg_v)
        same_state(state, state_v, f"D{D} greedy")
        return
    paths, r0 = [], 0
    for (_, ids, nd, par), (a, _, row, _) in zip(segs, got):           # the rows that stand: from `row` up the parents to the last certain row
        path = [row - r0] if a else []
        while path and par[path[0]] >= len(ids) - nd:
            path.insert(0, par[path[0]])
        paths.append(path)
        r0 += len(ids)
    print([r[0] for r in got])

    def draw(i, slot, fed, a):                                        # after A: the draw of step step0 + a from its last row
        return m.sample_rows([eng.pick_query(fed - 1, slot, seed=seeds[i], step=step0[i] + a, ban0=True, temp=0.4, top_p=0.6)])[0]
    held_to_alone(w, segs, paths, got, state, lg, f"D{D} nucleus", draw)
    for (_, ids, nd, par), path, (_, nx, _, _) in zip(segs, paths, got):      # the path ends where the draw names no child
        end = path[-1] if path else len(ids) - nd - 1
        assert nx not in [ids[r] for r in range(len(ids) - nd, len(ids)) if par[r] == end], "a child with the drawn id was left out"


def test_lookup_tree_streams_give_the_ids_of_lookup_streams(eng, models):
    m, w = models(*WIDTHS[0]).m, models(*WIDTHS[0])
    hist = [[3, 4, 5, 3, 4, 6, 3, 4], [9, 8, 9, 8, 9], [77]]           # two continuations behind "3 4", a cycle, nothing to look up
    restore(m, w.start)
    want, _ = m.decode_lookup_streams(hist, 12, k=6, n=2)
    restore(m, w.start)
    got, stats = m.decode_lookup_tree_streams(hist, 12, k=6, n=2, branches=3)
    assert got.tolist() == want.tolist() and all(st["rounds"] + st["accepted"] == 12 for st in stats)


@pytest.fixture(scope="module")
def guard_ctx(eng):
    ctx = GuardContexts(eng, 3, 64, MAXT)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("segs,ids,parent,pick,text", tc.REFUSED)
def test_refused_calls_leave_state_and_logits_as_they_were(eng, guard_ctx, segs, ids, parent, pick, text):
    n = len(segs)
    outs = ((C.c_uint32 * n)(), (C.c_uint64 * n)(), (C.c_uint64 * n)(), (C.c_uint64 * (eng.SPEC_MAX_DRAFT * n))())
    args = (guard_ctx.h["M"], *tc.refused_args(eng, segs, ids, parent))
    if pick is None:
        check_refused(guard_ctx, "rwkv_spec_verify_trees", (*args, 0, *outs), E_ARG, text)
    sampled = (eng.Pick * n)(*[eng.pick_of(**(pick or dict(temp=1.0, top_p=0.9)))] * n), (C.c_uint64 * n)(), (C.c_uint64 * n)()
    check_refused(guard_ctx, "rwkv_spec_sample_trees", (*args, *sampled, 0, *outs), E_ARG, text)
