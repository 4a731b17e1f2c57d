"""Segmented forward (include/rwkv_mi355x.h rwkv_forward_segments / rwkv_segment_plan): the cases of tests/test_segments_cpu.py and
tests/test_segments_gpu.py, a pure-Python STATEMENT of the call over any `forward(rows, state_of_one_slot)` -- run on the CPU oracle by the CPU
suite, compared with the device by the GPU suite -- and the Python statement of the row plan.

The models are modelfile.synthetic_tensors, every context loaded with max_ctx = 80.  Widths: those of spec_cases.WIDTHS -- 64 (the smallest chunk
width: WKV workgroups partly filled), 320 (uneven octants), 1024, and one 4096-wide two-layer case."""
import os

import numpy as np

V = 50277
MAXT = 80
PASS_ROWS = 64                                                 # what the exported rwkv_segment_plan assumes
WIDTHS = [(3, 64), (3, 320), (3, 1024), (2, 4096)]            # (layers, width)
SEED = 8100                                                    # + width: the models of the width cases
FIRST, LAST = 1, 2                                             # row_flags bits

# layouts as (slot, n) lists
LAYOUTS = dict(
    S2=[(0, 2)], S33=[(0, 33)], S65=[(0, 65)],                                 # one segment: one half, two halves, two passes
    MIX32=[(5, 1), (0, 7), (9, 1), (2, 23)],                                   # one half, singles next to runs
    MIX64=[(3, 30), (1, 4), (7, 1), (0, 29)],                                  # (1, 4) straddles the half boundary at row 32
    PAR40=[(s, 1) for s in range(40)],                                         # the PARRALEL layout, two halves
    MIX77=[(6, 60), (2, 10), (11, 1), (0, 1), (8, 5)],                         # (2, 10) straddles the pass boundary at row 64; two passes
    LAST=[(79, 1)],                                                            # one row on the last slot
)
ROWS = dict(S2=2, S33=33, S65=65, MIX32=32, MIX64=64, PAR40=40, MIX77=77, LAST=1)


def tokens_for(layout, seed):
    """[(slot, ids)] of a (slot, n) list: seeded ids in 1 .. V - 1"""
    rng = np.random.default_rng(seed)
    return [(s, [int(t) for t in rng.integers(1, V, n)]) for s, n in layout]


def last_rows(segments):
    out, j = [], 0
    for _, ids in segments:
        j += len(ids)
        out.append(j - 1)
    return out


def forward_segments(forward, state, segments):
    """the statement of rwkv_forward_segments over forward(rows, state_of_one_slot) -> logits [len(rows)][V], which runs the rows in GPT mode and
    advances the one-slot state (a list of five arrays) in place.  `state`: the five arrays xy, aa, bb, pp, dd over all slots, each of shape
    [slots][L * D], advanced in place.  Per segment: the slot is sliced out of the five arrays, the rows are run, the slot is written back.
    Returns the logits rows in packed order."""
    slots = [s for s, _ in segments]
    assert len(set(slots)) == len(slots), "the slots of one call are pairwise distinct"
    assert all(a.ndim == 2 for a in state)
    out = []
    for slot, ids in segments:
        one = [a[slot].copy() for a in state]
        out.append(np.asarray(forward([int(t) for t in ids], one)))
        for a, b in zip(state, one):
            a[slot] = b
    return np.concatenate(out, axis=0)


def segment_plan(layout, max_ctx, pass_rows=PASS_ROWS):
    """the statement of rwkv_segment_plan over a (slot, n) list: (row_slot, row_flags), or None where a rule is broken.  A piece ends where its
    segment ends or where the pass of `pass_rows` rows ends."""
    if len(layout) == 0 or any(n < 1 or not 0 <= s < max_ctx for s, n in layout):
        return None
    if len({s for s, _ in layout}) != len(layout) or not 1 <= sum(n for _, n in layout) <= max_ctx:
        return None
    slot, flags, j = [], [], 0
    for s, n in layout:
        for k in range(n):
            f = (FIRST if k == 0 or j % pass_rows == 0 else 0) | (LAST if k == n - 1 or (j + 1) % pass_rows == 0 else 0)
            slot.append(s); flags.append(f)
            j += 1
    return np.array(slot, np.uint32), np.array(flags, np.uint8)


def start_state(eng, m, D):
    """the state every GPU test starts from: a history on all 80 slots (80 seeded ids in PARRALEL mode), then a short GPT prompt on slot 0"""
    rng = np.random.default_rng(D)
    m.forward([int(v) for v in rng.integers(1, V, MAXT)], eng.MODE_PARRALEL)
    m.forward([7, 50000, 11, 9], eng.MODE_GPT)


def digest(m, n_rows):
    """SHA-256 over the five state arrays of all slots and logits rows 0 .. n_rows - 1, as the device holds them"""
    import hashlib
    m.pull_state(MAXT)
    h = hashlib.sha256()
    for a in m.state.arrays():
        h.update(np.ascontiguousarray(a).tobytes())
    h.update(np.ascontiguousarray(m.logits(n_rows)).tobytes())
    return h.hexdigest()


def mix77_digests(eng):
    """{width: digest} of MIX77 from the start state at every width -- in this process, whatever RWKV_SEQ_STAGES / RWKV_SEQ_ROWS it was started with
    (both are read when a context is created or first runs two passes)"""
    from rwkv_cpp_accelerated_amd import modelfile as mf
    out = {}
    for L, D in WIDTHS:
        m = eng.RWKV(resident=True)
        m.loadTensors(L, D, mf.synthetic_tensors(L, D, seed=SEED + D), maxGPT=MAXT)
        start_state(eng, m, D)
        m.forward_segments(tokens_for(LAYOUTS["MIX77"], 77 + D))
        out[D] = digest(m, ROWS["MIX77"])
        m.close()
    return out


if __name__ == "__main__":      # the child process of tests/test_segments_gpu.py: "D digest" per width, under the environment it was given
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from rwkv_cpp_accelerated_amd import engine
    for width, dg in mix77_digests(engine).items():
        print(width, dg)
