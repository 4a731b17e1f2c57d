"""Speculative greedy decoding for many streams on the device (include/rwkv_mi355x.h rwkv_spec_verify_segments, csrc/specseg.hip.h): the rollback
is EXACT per segment.  The reference continuation of every slot is built with rwkv_forward_segments alone, and what a verify leaves -- ids, slot
state, logits rows up to the committed row -- is held bit for bit to rwkv_forward_segments of the rows that stand, alone, from the same start.
One case is held to the f64 oracle within the chunk suite's bounds.  Every context has max_ctx = 80 and a history on all 80 slots."""
import ctypes as C

import numpy as np
import pytest

from rwkv_cpp_accelerated_amd import modelfile as mf
import parity
import segment_cases as sg
import spec_cases as sc
import specseg_cases as cs
from support import E_ARG, E_STATE, NAMES, GuardContexts, check_refused, eng, load, restore, rows, same_state, snapshot  # noqa: F401

pytestmark = pytest.mark.gpu
V, MAXT = cs.V, cs.MAXT


class Width:
    """one model with its start state and, per layout, the segments and the expected triples (once per module)"""

    def __init__(self, eng, L, D):
        self.t = mf.synthetic_tensors(L, D, seed=cs.SEED + D)
        self.m = load(eng, L, D, 0, MAXT, self.t)
        sg.start_state(eng, self.m, D)
        self.start, self.cases = snapshot(self.m, MAXT), {}

    def alone(self, slot, ids):
        """(state, logits rows) that rwkv_forward_segments of one segment leaves from the start state"""
        restore(self.m, self.start)
        self.m.forward_segments([(slot, ids)])
        return snapshot(self.m, MAXT), rows(self.m, len(ids))

    def case(self, name):
        if name not in self.cases:      # step j: every segment's certain ids and its first j greedy ids, from the start state
            lay = cs.LAYOUTS[name]
            g = [[] for _ in lay]
            for j in range(1 + max(nd for _, _, nd, _ in lay)):
                live = [i for i, s in enumerate(lay) if s[2] >= j]
                restore(self.m, self.start)
                last = self.m.forward_segments([(lay[i][0], cs.certain(lay[i][0], lay[i][1] - lay[i][2]) + g[i]) for i in live])
                lg = self.m.logits(last[-1] + 1).reshape(-1, V)
                for i, r in zip(live, last):
                    g[i].append(sc.pick(lg[r]))
            self.cases[name] = cs.plant(lay, g) + (g,)
        return self.cases[name]


@pytest.fixture(scope="module")
def widths(eng):
    cache = {}

    def get(L, D):
        if (L, D) not in cache:
            cache[(L, D)] = Width(eng, L, D)
        return cache[(L, D)]
    yield get
    for w in cache.values():
        w.m.close()


def held_to_forward_segments(w, segs, got, state, lg, what):
    """every named slot and its logits rows up to the committed row against rwkv_forward_segments of the rows that stand, alone"""
    r0 = 0
    for (slot, ids, nd), (a, _, row) in zip(segs, got):
        keep = len(ids) - nd + a
        assert row == r0 + keep - 1, what
        alone, alone_rows = w.alone(slot, ids[:keep])
        for k, name in enumerate(NAMES):
            assert np.array_equal(state[k][slot], alone[k][slot]), f"{what} slot {slot}: {name}"
        assert np.array_equal(lg[r0:r0 + keep], alone_rows), f"{what} slot {slot}: logits rows {r0} .. {row}"
        r0 += len(ids)


@pytest.mark.parametrize("name", list(cs.LAYOUTS))
@pytest.mark.parametrize("L,D", cs.WIDTHS)
def test_rollback_is_exact(eng, widths, L, D, name):
    w = widths(L, D)
    m, (segs, want, _) = w.m, w.case(name)
    restore(m, w.start)
    got = m.spec_verify_segments(segs)
    what = f"D{D} {name}"
    assert got == want, what
    state, lg = snapshot(m, MAXT), rows(m, sum(len(ids) for _, ids, _ in segs))
    same_state(state, w.start, what + ", slots not named", [s for s in range(MAXT) if s not in [x[0] for x in segs]])
    assert np.array_equal(state[3], w.start[3]), what + ": pp"
    held_to_forward_segments(w, segs, got, state, lg, what)
    if name.startswith("ONE"):                                        # {0, n, n - 1}: rwkv_spec_verify, bit for bit
        (_, ids, _), (a, nx, _) = segs[0], got[0]
        restore(m, w.start)
        assert m.spec_verify(ids[0], ids[1:]) == (a, nx), what
        same_state(snapshot(m, MAXT), state, what + " against spec_verify")
        assert np.array_equal(rows(m, a + 1), lg[:a + 1]), what + " against spec_verify: logits rows"


@pytest.mark.parametrize("L,D", cs.WIDTHS)
def test_two_calls_chain_like_one_forward(eng, widths, L, D):
    w = widths(L, D)
    m, (segs, want, g) = w.m, w.case("FIVE")
    restore(m, w.start)
    first = m.spec_verify_segments(segs)
    # the second call feeds `next` and, as its draft, the rest of the slot's continuation: all of it stands
    second = [(slot, [nx] + gi[a + 1:nd + 1], nd - a) for (slot, _, nd), (a, nx, _), gi in zip(segs, first, g)]
    assert [r[0] for r in m.spec_verify_segments(second)] == [nd for _, _, nd in second]
    state = snapshot(m, MAXT)
    for (slot, n, nd, _), gi in zip(cs.FIVE, g):
        alone, _ = w.alone(slot, cs.certain(slot, n - nd) + gi[:nd + 1])
        for k, name in enumerate(NAMES):
            assert np.array_equal(state[k][slot], alone[k][slot]), f"D{D} slot {slot}: {name}"


@pytest.mark.parametrize("L,D", cs.WIDTHS)
def test_against_the_statement_over_the_oracle(eng, oracle, widths, L, D):
    w = widths(L, D)
    m, (segs, _, _) = w.m, w.case("FIVE")
    restore(m, w.start)
    got = m.spec_verify_segments(segs)
    state, lg = snapshot(m, MAXT), rows(m, sum(len(ids) for _, ids, _ in segs))
    om = oracle.from_tensors(L, D, w.t)
    for (slot, ids, nd), (a, nx, row) in zip(segs, got):
        st = [s.view(np.float64)[slot].copy() for s in w.start]
        a_ref, nx_ref, l_ref, gmin = cs.oracle_verify(om.forward, st, ids, nd)
        what = f"D{D} slot {slot}"
        print(f"{what}: a {a} next {nx}, oracle a {a_ref} next {nx_ref}, smallest top-two gap {gmin:.2e}")
        assert gmin >= cs.MARGIN, what                                # (tests/test_specseg_cpu.py proves it on the oracle alone)
        assert (a, nx) == (a_ref, nx_ref), what
        for l in range(L):
            lo = slice(l * D, (l + 1) * D)
            for k, tol in ((0, parity.TOL), (1, 1e-4), (2, 1e-4), (4, parity.TOL)):
                parity._close(state[k].view(np.float64)[slot][lo], st[k][lo], f"{what} layer {l} {NAMES[k]}", tol)
        parity.check_logits(lg[row].view(np.float32), l_ref, what + " committed row")
    om.close()


GUARDS = [      # (context, segments (slot, n, n_draft, reserved), ids or None, flags, the NULL output or None, status, text)
    ("M", [(1, 2, 1, 0), (1, 2, 1, 0)], None, 0, None, E_ARG, "named twice"),
    ("M", [(0, 2, 2, 0)], None, 0, None, E_ARG, "n_draft 2 must be in 0..1"),
    ("M", [(0, 40, 32, 0)], None, 0, None, E_ARG, "n_draft 32 must be in 0..31"),
    ("M", [(0, 40, 0, 0), (1, 30, 0, 0)], None, 0, None, E_ARG, "ONE pass"),
    ("M", [(0, 40, 0, 0), (1, 41, 0, 0)], None, 0, None, E_ARG, "Context too large"),
    ("M", [(0, 2, 1, 0)], [5, V], 0, None, E_ARG, f"token id {V} out of range"),
    ("M", [(0, 2, 1, 1)], None, 0, None, E_ARG, "reserved must be 0"),
    ("M", [(0, 2, 1, 0)], None, 1, None, E_ARG, "flags must be 0"),
    ("M", [(0, 2, 1, 0)], None, 0, 0, E_ARG, "NULL"),
    ("M", [(0, 2, 1, 0)], None, 0, 1, E_ARG, "NULL"),
    ("S", [(0, 2, 1, 0)], None, 0, None, E_STATE, "whole-model"),
]


@pytest.fixture(scope="module")
def guard_ctx(eng):
    ctx = GuardContexts(eng, 3, 64, MAXT)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("who,segs,ids,flags,null,status,text", GUARDS)
def test_refused_calls_leave_state_and_logits_as_they_were(eng, guard_ctx, who, segs, ids, flags, null, status, text):
    T = sum(s[1] for s in segs)
    outs = [(C.c_uint32 * 64)(), (C.c_uint64 * 64)(), (C.c_uint64 * 64)()]
    if null is not None:
        outs[null] = None
    args = (guard_ctx.h[who], (C.c_uint64 * T)(*(ids or [5] * T)), (eng.SpecSegment * len(segs))(*[eng.SpecSegment(*s) for s in segs]), len(segs), flags, *outs)
    check_refused(guard_ctx, "rwkv_spec_verify_segments", args, status, text)
