"""Segmented forward on the device (include/rwkv_mi355x.h rwkv_forward_segments, csrc/segments.hip.h): the result for a segment is EXACT -- bit
for bit what the same segment alone in a call leaves, and, for one segment on slot 0, what rwkv_forward(GPT) leaves -- whatever else the call
holds, wherever the rows sit in their pass and however the rows are cut into passes.  The oracle check holds the logits to parity.check_logits
and aa / bb to the chunk suite's 1e-4 of the vector's max |.|.  Every context has max_ctx = 80 and every test starts from a saved state with
history on all 80 slots (tests/segment_cases.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from rwkv_cpp_accelerated_amd import modelfile as mf
import parity
import segment_cases as sg
from support import E_ARG, E_STATE, NAMES, build_app, eng, load, restore, rows, same_state, snapshot  # noqa: F401

pytestmark = pytest.mark.gpu
V, MAXT = sg.V, sg.MAXT


class Width:
    """one model of the width cases with its start state (once per module)"""

    def __init__(self, eng, L, D):
        self.L, self.D = L, D
        self.t = mf.synthetic_tensors(L, D, seed=sg.SEED + D)
        self.m = load(eng, L, D, 0, MAXT, self.t)
        sg.start_state(eng, self.m, D)
        self.start = snapshot(self.m, MAXT)
        for x in self.start:
            x.setflags(write=False)

    def run(self, segments):
        """(state, logits rows, last_row) of one call from the start state"""
        restore(self.m, self.start)
        last = self.m.forward_segments(segments)
        return snapshot(self.m, MAXT), rows(self.m, sum(len(ids) for _, ids in segments)), last

    def close(self):
        self.m.close()


@pytest.fixture(scope="module")
def widths(eng):
    cache = {}

    def get(L, D):
        if (L, D) not in cache:
            cache[(L, D)] = Width(eng, L, D)
        return cache[(L, D)]
    yield get
    for w in cache.values():
        w.close()


@pytest.mark.parametrize("L,D", sg.WIDTHS)
def test_one_segment_is_gpt_mode_bit_for_bit(eng, widths, L, D):
    w = widths(L, D)
    m = w.m
    for name in ("S2", "S33", "S65"):
        (_, ids), = sg.tokens_for(sg.LAYOUTS[name], D + len(name))
        n = len(ids)
        restore(m, w.start)
        m.forward(ids, eng.MODE_GPT)
        want, want_rows = snapshot(m, MAXT), rows(m, n)
        got, got_rows, last = w.run([(0, ids)])
        what = f"D{D} {name}"
        assert last == [n - 1], what
        same_state(got, want, what)
        assert np.array_equal(got_rows, want_rows), what + ": logits rows"
        # the same segment on slot 41, which holds a copy of slot 0: slot 41 gets the bits slot 0 got, every other slot stays
        restore(m, w.start)
        m.copy_state(41, 0)
        base = snapshot(m, MAXT)
        assert m.forward_segments([(41, ids)]) == [n - 1]
        got = snapshot(m, MAXT)
        others = [s for s in range(MAXT) if s != 41]
        same_state(got, base, what + " on slot 41, the other slots", others)
        for k, name_k in enumerate(NAMES):
            assert np.array_equal(got[k][41], want[k][0]), f"{what} on slot 41: {name_k}"
        assert np.array_equal(rows(m, n), want_rows), what + " on slot 41: logits rows"
    # one row on slot 0 is the one-row pass of the chunk path
    restore(m, w.start)
    m.spec_verify(4242, [])
    want, want_row = snapshot(m, MAXT), rows(m, 1)
    got, got_row, last = w.run([(0, [4242])])
    assert last == [0]
    same_state(got, want, f"D{D} (0, 1) against spec_verify")
    assert np.array_equal(got_row, want_row)


@pytest.mark.parametrize("name", ["MIX32", "MIX64", "MIX77", "LAST"])
@pytest.mark.parametrize("L,D", sg.WIDTHS)
def test_a_segment_does_not_depend_on_the_rest_of_the_call(eng, widths, L, D, name):
    w = widths(L, D)
    segs = sg.tokens_for(sg.LAYOUTS[name], sg.ROWS[name] + D)
    got, got_rows, last = w.run(segs)
    what = f"D{D} {name}"
    assert last == sg.last_rows(segs), what
    named = [s for s, _ in segs]
    others = [s for s in range(MAXT) if s not in named]
    same_state(got, w.start, what + ", slots not named", others)
    assert np.array_equal(got[3], w.start[3]), what + ": pp"           # the chunk path does not use it
    row = 0
    for slot, ids in segs:
        alone, alone_rows, _ = w.run([(slot, ids)])
        for k, name_k in enumerate(NAMES):
            assert np.array_equal(got[k][slot], alone[k][slot]), f"{what} slot {slot}: {name_k}"
        assert np.array_equal(got_rows[row:row + len(ids)], alone_rows), f"{what} slot {slot}: logits rows {row} .. {row + len(ids) - 1}"
        row += len(ids)


def test_pass_cutting_and_stage_count_do_not_change_a_bit(eng):
    """MIX77 at every width in a child process under RWKV_SEQ_STAGES=1 (both passes on one stream) and under RWKV_SEQ_ROWS=32 (three passes, the
    pieces cut at rows 32 and 64): both are read when a context is created or first runs two passes"""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "segment_cases.py")
    children = {}
    for var, val in (("RWKV_SEQ_STAGES", "1"), ("RWKV_SEQ_ROWS", "32")):          # both at once, next to this process's own run
        children[var] = subprocess.Popen([sys.executable, script], env=dict(os.environ, **{var: val}), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    here = sg.mix77_digests(eng)
    done = {var: p.communicate(timeout=120) for var, p in children.items()}      # (both have ended before anything is asserted)
    for var, (out, err) in done.items():
        assert children[var].returncode == 0, (var, out, err)
        there = {int(l.split()[0]): l.split()[1] for l in out.splitlines() if len(l.split()) == 2 and l.split()[0].isdigit()}
        print(var, there)
        assert there == here, var


@pytest.mark.parametrize("L,D", sg.WIDTHS)
def test_two_calls_chain_like_one(eng, widths, L, D):
    w = widths(L, D)
    segs = sg.tokens_for(sg.LAYOUTS["MIX64"], 64 + D)
    more = sg.tokens_for([(s, 3) for s, _ in sg.LAYOUTS["MIX64"]], 3 + D)
    restore(w.m, w.start)
    w.m.forward_segments(segs)
    last2 = w.m.forward_segments(more)
    got, got_rows = snapshot(w.m, MAXT), rows(w.m, 12)
    longer = [(s, a + b) for (s, a), (_, b) in zip(segs, more)]
    want, want_rows, last = w.run(longer)
    same_state(got, want, f"D{D} MIX64 then 3 more per slot")
    assert last2 == [2, 5, 8, 11]
    for i, r in enumerate(last):                                     # the three rows each segment got in the second call
        assert np.array_equal(got_rows[3 * i:3 * i + 3], want_rows[r - 2:r + 1]), (D, i)


@pytest.mark.parametrize("name", ["MIX64", "PAR40"])
@pytest.mark.parametrize("L,D", sg.WIDTHS)
def test_against_the_statement_over_the_oracle(eng, oracle, widths, L, D, name):
    w = widths(L, D)
    segs = sg.tokens_for(sg.LAYOUTS[name], sg.ROWS[name] + 2 * D)
    got, got_rows, _ = w.run(segs)
    om = oracle.from_tensors(L, D, w.t)
    st = [s.view(np.float64).copy() for s in w.start]
    ref = sg.forward_segments(om.forward, st, segs)
    om.close()
    what = f"D{D} {name}"
    e = parity.check_logits(got_rows.view(np.float32), ref, what + " logits")
    print(f"{what}: logits max |d| / max |ref| = {e:.2e}")
    for slot, _ in segs:
        for k in (1, 2):
            for l in range(L):
                lo = slice(l * D, (l + 1) * D)
                parity._close(got[k].view(np.float64)[slot][lo], st[k][slot][lo], f"{what} slot {slot} layer {l} {NAMES[k]}", 1e-4)
    if name == "PAR40":                                              # against rwkv_forward(PARRALEL): the bound is asserted, bit equality is reported
        restore(w.m, w.start)
        w.m.forward([ids[0] for _, ids in segs], eng.MODE_PARRALEL)
        par, par_rows = snapshot(w.m, MAXT), rows(w.m, 40)
        parity.check_logits(got_rows.view(np.float32), par_rows.view(np.float32), what + " against forward(PARRALEL)")
        eq = {n_: bool(np.array_equal(g, p)) for n_, g, p in zip(NAMES, got, par)}
        print(f"{what} against rwkv_forward(PARRALEL): state bitwise equal {eq}, logits bitwise equal {bool(np.array_equal(got_rows, par_rows))}")


def test_refused_calls_leave_state_and_logits_as_they_were(eng, widths):
    L, D = sg.WIDTHS[0]
    w = widths(L, D)
    m, lib = w.m, eng.lib()
    u64 = C.c_uint64
    ids = lambda *v: (u64 * len(v))(*v)
    sl = lambda *v: (eng.Segment * len(v))(*[eng.Segment(s, n) for s, n in v])
    t = mf.synthetic_tensors(2, 64, seed=1)
    ctx = dict(M=m, U=eng.RWKV(resident=True), S=eng.RWKV(resident=True), N=eng.RWKV(resident=True))
    ctx["S"].set_layer_range(0, 1)
    ctx["S"].loadTensors(2, 64, t, maxGPT=MAXT)
    ctx["N"].loadTensors(2, 64, t, maxGPT=1)                          # no chunk path: max context 1
    h = {k: v._h for k, v in ctx.items()}
    last = (u64 * 8)()
    many = ids(*[5] * (MAXT + 1))
    cases = [
        (("M", None, sl((0, 2)), 1, 0, last), E_ARG, "NULL"),
        (("M", ids(5, 6), None, 1, 0, last), E_ARG, "NULL"),
        (("M", ids(5, 6), sl((0, 2)), 0, 0, last), E_ARG, "n_segs must be in 1.."),
        (("M", ids(5, 6), sl((0, 1), (0, 1)), 2, 0, last), E_ARG, "named twice"),
        (("M", ids(5, 6), sl((0, 2), (3, 0)), 2, 0, last), E_ARG, "is empty"),
        (("M", ids(5, 6), sl((MAXT, 2)), 1, 0, last), E_ARG, "out of range"),
        (("M", many, sl((0, 40), (1, 41)), 2, 0, last), E_ARG, "Context too large"),
        (("M", ids(5, V), sl((0, 1), (1, 1)), 2, 0, last), E_ARG, f"token id {V} out of range"),
        (("M", ids(5, 6), sl((0, 2)), 1, 1, last), E_ARG, "flags must be 0"),
        (("U", ids(5, 6), sl((0, 2)), 1, 0, last), E_STATE, "RWKV not loaded"),
        (("S", ids(5, 6), sl((0, 2)), 1, 0, last), E_STATE, "whole-model"),
        (("N", ids(5), sl((0, 1)), 1, 0, last), E_STATE, "chunked path not available"),
    ]
    restore(m, w.start)
    m.forward_segments([(3, [5, 6, 7]), (0, [8])])                    # four logits rows and a state to keep
    state, logits = snapshot(m, MAXT), rows(m, MAXT)
    for args, status, text in cases:
        rc = int(lib.rwkv_forward_segments(*[h[v] if isinstance(v, str) else v for v in args]))
        err = lib.rwkv_last_error().decode()
        print(f"{args[0]}: status {rc}, {err!r}")
        assert rc == status and text in err, (args, err)
        same_state(snapshot(m, MAXT), state, text)
        assert np.array_equal(rows(m, MAXT), logits), text
    assert lib.rwkv_forward_segments(h["M"], ids(5, 6), sl((0, 2)), 1, 0, None) == 0       # last_row may be NULL
    for k, v in ctx.items():
        if k != "M":
            v.close()


def test_host_authoritative_state_is_pushed_and_pulled(eng, widths):
    """resident=False: the binding pushes slots 0 .. the largest slot named before the call and pulls them after"""
    L, D = sg.WIDTHS[0]
    w = widths(L, D)
    segs = sg.tokens_for(sg.LAYOUTS["MIX32"], 32)
    want, want_rows, want_last = w.run(segs)
    h = eng.RWKV(resident=False)
    h.loadTensors(L, D, w.t, maxGPT=MAXT)
    for a, b in zip(h.state.arrays(), w.start):
        a.reshape(-1)[:] = b.view(np.float64).reshape(-1)
    assert h.forward_segments(segs) == want_last
    top = 1 + max(s for s, _ in segs)
    for name, a, b, c in zip(NAMES, h.state.arrays(), want, w.start):
        got = a.view(np.uint64).reshape(MAXT, -1)
        assert np.array_equal(got[:top], b[:top]) and np.array_equal(got[top:], c[top:]), name
    assert np.array_equal(rows(h, 32), want_rows)
    h.close()


def test_segments_app_prints_the_engine_rows(eng, tmp_path):
    L, D = 3, 64
    t = mf.synthetic_tensors(L, D, seed=sg.SEED + 5)
    path = str(tmp_path / "model.bin")
    mf.write_bin(path, L, D, t)
    app = build_app("segments_app", tmp_path)
    r = subprocess.run([app, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("segments_ok"), (r.returncode, r.stdout, r.stderr)
    lines = [l.split() for l in r.stdout.splitlines() if l.startswith(("last", "argmax"))]
    assert [l[0] for l in lines] == ["last", "argmax", "last", "argmax"], r.stdout
    m = eng.RWKV(resident=True)
    m.loadTensors(L, D, t, maxGPT=MAXT)
    last = m.forward_segments([(0, [100]), (1, [5, 6, 7, 800, 9]), (2, list(range(11, 23)))])
    assert last == [0, 5, 17] == [int(v) for v in lines[0][1:]]
    a = [int(v) for v in m.score_rows(last, [1, 1, 1])[2]]
    assert a == [int(v) for v in lines[1][1:]]
    last = m.forward_segments([(2, [a[2]]), (0, [a[0]]), (1, [a[1]])])
    assert last == [0, 1, 2] == [int(v) for v in lines[2][1:]]
    assert [int(v) for v in m.score_rows(last, [1, 1, 1])[2]] == [int(v) for v in lines[3][1:]]
    m.close()
