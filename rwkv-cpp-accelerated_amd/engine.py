"""ctypes binding of librwkv_mi355x.so (include/rwkv_mi355x.h) and a Python mirror of the
reference's host class `RWKV` (include/rwkv/rwkv/rwkv.h:245-429).

Nothing here computes: every forward goes through the C-ABI into the HIP kernels.  There is no
CPU fallback -- if the shared library is missing or no HIP device is present the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import modelfile as mf

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RWKV_LIB") or os.path.join(_HERE, "csrc", "librwkv_mi355x.so")   # RWKV_LIB: tuning variants

MODE_PARRALEL, MODE_GPT = 0, 1   # reference enums/enum.h:2-5
SAMPLE_BAN0, SAMPLE_RECIPE = 1, 2   # include/rwkv_mi355x.h
NUCLEUS_BAN0, NUCLEUS_KEEP, NUCLEUS_UPDATE = 1, 2, 4
STOP_MAX_SEQS, STOP_MAX_LEN, STOP_POLL, STOP_KEEP = 16, 8, 8, 1
PICK_GREEDY, PICK_TYPICAL, PICK_NUCLEUS = 0, 1, 2
N_KCLASS = 7
ABI_VERSION = 6                   # RWKV_MI355X_ABI_VERSION of include/rwkv_mi355x.h
KCLASS_NAMES = ["first", "att_kvr_wkv", "att_out", "ffn_rk", "ffn_v", "head", "argmax"]

# every entry point declared in include/rwkv_mi355x.h (tests check the library exports all of them)
ABI_SYMBOLS = [
    "rwkv_create", "rwkv_load_file", "rwkv_load_tensors", "rwkv_n_layers", "rwkv_n_embed", "rwkv_max_ctx",
    "rwkv_forward", "rwkv_set_state", "rwkv_get_output", "rwkv_reset_state", "rwkv_decode_greedy",
    "rwkv_free", "rwkv_last_error", "rwkv_logits_device", "rwkv_state_device", "rwkv_stream",
    "rwkv_bytes_per_token", "rwkv_profile_token", "rwkv_debug_launch", "rwkv_debug_read", "rwkv_debug_write", "rwkv_debug_grid", "rwkv_debug_timeline", "rwkv_profile_batched", "rwkv_abi_version", "rwkv_resident_bytes", "rwkv_decode_form", "rwkv_set_layer_range", "rwkv_stage_forward", "rwkv_x_device", "rwkv_sample_typical", "rwkv_decode_typical",
    "rwkv_stage_chunk", "rwkv_xseq_device", "rwkv_xseq_copy", "rwkv_sync", "rwkv_pipe_rccl_path", "rwkv_pipe_unique_id", "rwkv_pipe_init", "rwkv_pipe_decode", "rwkv_pipe_decode_streams", "rwkv_pipe_profile", "rwkv_pipe_hop_stats",
    "rwkv_pipe_prefill", "rwkv_pipe_free", "rwkv_tensor_device", "rwkv_pipe_info", "rwkv_pipe_decode_dual",
    "rwkv_decode_batch_greedy", "rwkv_decode_batch_typical", "rwkv_state_copy",
    "rwkv_score_rows", "rwkv_score",
    "rwkv_sample_nucleus", "rwkv_decode_nucleus", "rwkv_decode_batch_nucleus", "rwkv_penalty_set", "rwkv_penalty_get",
    "rwkv_decode_batch_until", "rwkv_debug_stop_scan",
    "rwkv_topn_rows", "rwkv_decode_batch_logprobs",
    "rwkv_decode_beam", "rwkv_state_permute", "rwkv_debug_beam_step",
    "rwkv_constraint_set", "rwkv_constraint_clear", "rwkv_constraint_state_set", "rwkv_constraint_state_get", "rwkv_pick_constrained",
    "rwkv_debug_constrained_row", "rwkv_decode_batch_constrained",
    "rwkv_spec_verify", "rwkv_decode_speculative",
    "rwkv_forward_segments", "rwkv_segment_plan",
]
CONSTRAINT_MAX_STATES, CONSTRAINT_MAX_EDGES, CONSTRAINT_MAX_BIAS, STOP_CONSTRAINT = 4096, 1 << 24, 300, 32   # RWKV_CONSTRAINT_*, RWKV_STOP_CONSTRAINT
BEAM_MAX, BEAM_MAX_STOP = 16, 16  # RWKV_MAX_BEAM, RWKV_BEAM_MAX_STOP
SPEC_MAX_DRAFT = 31               # RWKV_SPEC_MAX_DRAFT
MAX_SCORE = 65536                 # RWKV_MAX_SCORE
TOPN_MAX = 32                     # RWKV_MAX_TOPN
LOGPROB_ENTRIES_MAX = 1 << 22     # RWKV_MAX_LOGPROB_ENTRIES: n_streams * n_steps * (1 + top_n) of one call

_lib = None


class NucleusParams(C.Structure):
    """rwkv_nucleus_params of include/rwkv_mi355x.h (32 bytes)"""
    _fields_ = [("temp", C.c_float), ("top_p", C.c_float), ("top_k", C.c_uint32), ("presence", C.c_float), ("frequency", C.c_float),
                ("decay", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


def nucleus_params(temp=1.0, top_p=0.9, top_k=0, presence=0.0, frequency=0.0, decay=1.0, flags=0) -> NucleusParams:
    return NucleusParams(float(temp), float(top_p), int(top_k), float(presence), float(frequency), float(decay), int(flags), 0)


class Pick(C.Structure):
    """rwkv_pick of include/rwkv_mi355x.h (48 bytes)"""
    _fields_ = [("kind", C.c_int), ("temp", C.c_float), ("tau", C.c_float), ("typical_flags", C.c_int), ("nucleus", NucleusParams)]


class StopParams(C.Structure):
    """rwkv_stop_params of include/rwkv_mi355x.h (40 bytes)"""
    _fields_ = [("seq_ids", C.POINTER(C.c_uint64)), ("seq_len", C.POINTER(C.c_uint32)), ("n_seqs", C.c_uint32), ("flags", C.c_uint32),
                ("max_new", C.POINTER(C.c_uint32)), ("reserved", C.c_uint64)]


def stop_params(sequences=(), max_new=None, keep=False):
    """(StopParams, the arrays it points into -- keep them alive for the call)"""
    seqs = [[int(t) for t in q] for q in sequences]
    flat = [t for q in seqs for t in q]
    ids = (C.c_uint64 * max(1, len(flat)))(*flat)
    lens = (C.c_uint32 * max(1, len(seqs)))(*[len(q) for q in seqs])
    mx = None if max_new is None else (C.c_uint32 * max(1, len(max_new)))(*[int(v) for v in max_new])
    sp = StopParams(ids if seqs else None, lens if seqs else None, len(seqs), STOP_KEEP if keep else 0, mx, 0)
    return sp, (ids, lens, mx)


class LogprobOut(C.Structure):
    """rwkv_logprob_out of include/rwkv_mi355x.h (40 bytes)"""
    _fields_ = [("top_n", C.c_uint32), ("reserved", C.c_uint32), ("logprob", C.POINTER(C.c_double)), ("entropy", C.POINTER(C.c_double)),
                ("top_ids", C.POINTER(C.c_uint64)), ("top_logprob", C.POINTER(C.c_double))]


class BeamParams(C.Structure):
    """rwkv_beam_params of include/rwkv_mi355x.h (24 bytes)"""
    _fields_ = [("width", C.c_uint32), ("n_stop", C.c_uint32), ("stop_ids", C.POINTER(C.c_uint64)), ("reserved", C.c_uint64)]


class BeamOut(C.Structure):
    """rwkv_beam_out of include/rwkv_mi355x.h (32 bytes)"""
    _fields_ = [("tokens", C.POINTER(C.c_uint64)), ("len", C.POINTER(C.c_uint32)), ("score", C.POINTER(C.c_double)),
                ("token_logprob", C.POINTER(C.c_double))]


def beam_params(width, stops=()):
    """(BeamParams, the array it points into -- keep it alive for the call)"""
    st = [int(t) for t in stops]
    ids = (C.c_uint64 * max(1, len(st)))(*st)
    return BeamParams(int(width), len(st), ids if st else None, 0), ids


class SpecStats(C.Structure):
    """rwkv_spec_stats of include/rwkv_mi355x.h (24 bytes)"""
    _fields_ = [("rounds", C.c_uint64), ("drafted", C.c_uint64), ("accepted", C.c_uint64)]


class Segment(C.Structure):
    """rwkv_segment of include/rwkv_mi355x.h (8 bytes)"""
    _fields_ = [("slot", C.c_uint32), ("n", C.c_uint32)]


def _segments(segments):
    """(Segment array, count, the packed ids) of a list of (slot, token_ids)"""
    segs = [(int(s), [int(t) for t in ids]) for s, ids in segments]
    arr = (Segment * max(1, len(segs)))(*[Segment(s, len(ids)) for s, ids in segs])
    return arr, len(segs), [t for _, ids in segs for t in ids]


def segment_plan(segments, max_ctx: int):
    """rwkv_segment_plan, host only (no model, no device): validates `segments`, a list of (slot, token_ids) or of (slot, n), against max_ctx and
    returns (row_slot, row_flags) for passes of 64 rows: per row of the call its slot, and bit 0 = first of its piece, bit 1 = last of its piece.
    A list that breaks a rule raises RWKVError."""
    segs = [(int(s), int(n) if np.isscalar(n) else len(n)) for s, n in segments]
    arr = (Segment * max(1, len(segs)))(*[Segment(s, n) for s, n in segs])
    T = C.c_uint64(0)
    _chk(lib().rwkv_segment_plan(arr, len(segs), int(max_ctx), None, None, C.byref(T)))
    slot, flags = np.zeros(T.value, np.uint32), np.zeros(T.value, np.uint8)
    _chk(lib().rwkv_segment_plan(arr, len(segs), int(max_ctx), slot.ctypes.data_as(C.POINTER(C.c_uint32)), flags.ctypes.data_as(C.POINTER(C.c_uint8)), None))
    return slot, flags


def ngram_draft(history, k: int, n: int = 3):
    """the host-side lookup drafter (no model): the up to k ids that followed the MOST RECENT earlier occurrence of the last n ids of `history`;
    [] where the history is shorter than n + 1 ids or its tail has not occurred before.  An occurrence may overlap the tail itself."""
    h = [int(t) for t in history]
    n, k = int(n), int(k)
    if n < 1 or k < 1 or len(h) <= n:
        return []
    tail = h[-n:]
    for s in range(len(h) - n - 1, -1, -1):           # the occurrence starts at s and ends in front of the last id: something follows it
        if h[s:s + n] == tail:
            return h[s + n:s + n + k]
    return []


class Automaton(C.Structure):
    """rwkv_automaton of include/rwkv_mi355x.h (40 bytes)"""
    _fields_ = [("n_states", C.c_uint32), ("reserved", C.c_uint32), ("nnz", C.c_uint64), ("row_ptr", C.POINTER(C.c_uint32)),
                ("tok", C.POINTER(C.c_uint32)), ("next", C.POINTER(C.c_uint32))]


class Bias(C.Structure):
    """rwkv_bias of include/rwkv_mi355x.h (24 bytes)"""
    _fields_ = [("n", C.c_uint32), ("reserved", C.c_uint32), ("tok", C.POINTER(C.c_uint32)), ("val", C.POINTER(C.c_float))]


class ConstrainParams(C.Structure):
    """rwkv_constrain_params of include/rwkv_mi355x.h (48 bytes)"""
    _fields_ = [("start", C.POINTER(C.c_uint32)), ("bias_ptr", C.POINTER(C.c_uint32)), ("bias_tok", C.POINTER(C.c_uint32)),
                ("bias_val", C.POINTER(C.c_float)), ("out_state", C.POINTER(C.c_uint32)), ("reserved", C.c_uint64)]


def _bias_arrays(bias):
    """one bias list -- a dict {id: value} or a sequence of (id, value) pairs, given in any order -- as (ids u32, values f32), ids ascending"""
    pairs = sorted((int(t), float(v)) for t, v in (bias.items() if hasattr(bias, "items") else bias))
    return np.array([t for t, _ in pairs], dtype=np.uint32), np.array([v for _, v in pairs], dtype=np.float32)


def constraint_trie(choices):
    """(row_ptr, tok, next) u32: the automaton that spells exactly one of the token sequences `choices` -- a trie with shared prefixes merged, state
    0 the root, the states numbered in the order the choices first reach them, every leaf terminal (include/rwkv_sampler.h constraint_trie builds
    the same arrays).  A stream ends where it reaches a state WITHOUT edges: a choice that is a proper prefix of another one is accepted as a
    path, but a stream that follows it goes on to one of its extensions.  Empty choices and ids outside 1 .. 50276 are skipped."""
    kids = [dict()]
    for ch in choices:
        ch = [int(t) for t in ch]
        if not ch or any(t < 1 or t >= mf.VOCAB for t in ch):
            continue
        q = 0
        for t in ch:
            if t not in kids[q]:
                kids[q][t] = len(kids)
                kids.append(dict())
            q = kids[q][t]
    row_ptr, tok, nxt = [0], [], []
    for k in kids:
        for t in sorted(k):
            tok.append(t); nxt.append(k[t])
        row_ptr.append(len(tok))
    return np.array(row_ptr, np.uint32), np.array(tok, np.uint32), np.array(nxt, np.uint32)


class RWKVError(RuntimeError):
    pass


def lib():
    """dlopen the engine; fail loudly when it has not been built (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RWKVError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(LIB_PATH)
    vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
    L.rwkv_create.argtypes = [C.POINTER(vp), i32]; L.rwkv_create.restype = i32
    L.rwkv_load_file.argtypes = [vp, C.c_char_p, u64]; L.rwkv_load_file.restype = i32
    L.rwkv_load_tensors.argtypes = [vp, u64, u64, C.POINTER(vp), i32, u64]; L.rwkv_load_tensors.restype = i32
    for f in ("rwkv_n_layers", "rwkv_n_embed", "rwkv_max_ctx", "rwkv_bytes_per_token"):
        getattr(L, f).argtypes = [vp]; getattr(L, f).restype = u64
    L.rwkv_forward.argtypes = [vp, C.POINTER(u64), u64, i32]; L.rwkv_forward.restype = i32
    L.rwkv_set_state.argtypes = [vp] + [vp] * 5 + [u64]; L.rwkv_set_state.restype = i32
    L.rwkv_get_output.argtypes = [vp] + [vp] * 6 + [u64]; L.rwkv_get_output.restype = i32
    L.rwkv_reset_state.argtypes = [vp]; L.rwkv_reset_state.restype = i32
    L.rwkv_decode_greedy.argtypes = [vp, u64, u64, C.POINTER(u64)]; L.rwkv_decode_greedy.restype = i32
    L.rwkv_free.argtypes = [vp]; L.rwkv_free.restype = None
    L.rwkv_last_error.argtypes = []; L.rwkv_last_error.restype = C.c_char_p
    L.rwkv_logits_device.argtypes = [vp]; L.rwkv_logits_device.restype = vp
    L.rwkv_state_device.argtypes = [vp, i32]; L.rwkv_state_device.restype = vp
    L.rwkv_stream.argtypes = [vp]; L.rwkv_stream.restype = vp
    L.rwkv_profile_token.argtypes = [vp, u64, i32, C.POINTER(C.c_double), C.POINTER(u64), C.POINTER(C.c_uint32)]
    L.rwkv_profile_token.restype = i32
    L.rwkv_debug_launch.argtypes = [vp, i32, u64, u64, C.c_uint32]; L.rwkv_debug_launch.restype = i32
    L.rwkv_debug_read.argtypes = [vp, i32, vp, u64]; L.rwkv_debug_read.restype = i32
    L.rwkv_debug_write.argtypes = [vp, i32, vp, u64]; L.rwkv_debug_write.restype = i32
    L.rwkv_debug_grid.argtypes = [vp]; L.rwkv_debug_grid.restype = u64
    L.rwkv_set_layer_range.argtypes = [vp, u64, u64]; L.rwkv_set_layer_range.restype = i32
    L.rwkv_stage_forward.argtypes = [vp, u64, C.c_uint32, C.POINTER(u64)]; L.rwkv_stage_forward.restype = i32
    L.rwkv_x_device.argtypes = [vp]; L.rwkv_x_device.restype = vp
    L.rwkv_profile_batched.argtypes = [vp, u64, i32, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]; L.rwkv_profile_batched.restype = i32
    L.rwkv_debug_timeline.argtypes = [vp, u64, vp, u64]; L.rwkv_debug_timeline.restype = i32
    L.rwkv_abi_version.argtypes = []; L.rwkv_abi_version.restype = i32
    L.rwkv_resident_bytes.argtypes = [vp]; L.rwkv_resident_bytes.restype = u64
    L.rwkv_decode_form.argtypes = [vp]; L.rwkv_decode_form.restype = i32
    if L.rwkv_abi_version() != ABI_VERSION:
        raise RWKVError(f"{LIB_PATH} has C-ABI version {L.rwkv_abi_version()}, this binding expects {ABI_VERSION}: rebuild it")
    L.rwkv_sample_typical.argtypes = [vp, u64, C.c_float, C.c_float, C.c_double, i32, C.POINTER(u64)]; L.rwkv_sample_typical.restype = i32
    L.rwkv_decode_typical.argtypes = [vp, u64, u64, C.c_float, C.c_float, u64, i32, C.POINTER(u64)]; L.rwkv_decode_typical.restype = i32
    L.rwkv_stage_chunk.argtypes = [vp, C.POINTER(u64), u64, u64, i32]; L.rwkv_stage_chunk.restype = i32
    L.rwkv_xseq_device.argtypes = [vp, i32]; L.rwkv_xseq_device.restype = vp
    L.rwkv_xseq_copy.argtypes = [vp, i32, vp, i32, u64]; L.rwkv_xseq_copy.restype = i32
    L.rwkv_sync.argtypes = [vp]; L.rwkv_sync.restype = i32
    L.rwkv_pipe_rccl_path.argtypes = [C.c_char_p, u64]; L.rwkv_pipe_rccl_path.restype = i32
    L.rwkv_pipe_unique_id.argtypes = [vp]; L.rwkv_pipe_unique_id.restype = i32
    L.rwkv_pipe_init.argtypes = [vp, vp, i32, i32]; L.rwkv_pipe_init.restype = i32
    L.rwkv_pipe_decode.argtypes = [vp, C.POINTER(u64), u64, C.POINTER(u64)]; L.rwkv_pipe_decode.restype = i32
    L.rwkv_pipe_decode_streams.argtypes = [vp, C.POINTER(u64), u64, u64, C.POINTER(u64)]; L.rwkv_pipe_decode_streams.restype = i32
    L.rwkv_pipe_profile.argtypes = [vp, i32]; L.rwkv_pipe_profile.restype = i32
    L.rwkv_pipe_hop_stats.argtypes = [vp, C.POINTER(C.c_double)]; L.rwkv_pipe_hop_stats.restype = i32
    L.rwkv_pipe_prefill.argtypes = [vp, C.POINTER(u64), u64]; L.rwkv_pipe_prefill.restype = i32
    L.rwkv_pipe_free.argtypes = [vp]; L.rwkv_pipe_free.restype = None
    L.rwkv_pipe_info.argtypes = [vp, C.c_char_p, u64]; L.rwkv_pipe_info.restype = i32
    L.rwkv_pipe_decode_dual.argtypes = [vp, C.POINTER(u64), u64, C.POINTER(u64)]; L.rwkv_pipe_decode_dual.restype = i32
    L.rwkv_tensor_device.argtypes = [vp, i32]; L.rwkv_tensor_device.restype = vp
    L.rwkv_decode_batch_greedy.argtypes = [vp, C.POINTER(u64), u64, u64, C.POINTER(u64)]; L.rwkv_decode_batch_greedy.restype = i32
    L.rwkv_decode_batch_typical.argtypes = [vp, C.POINTER(u64), u64, u64, C.c_float, C.c_float, C.POINTER(u64), i32, C.POINTER(u64)]
    L.rwkv_decode_batch_typical.restype = i32
    L.rwkv_state_copy.argtypes = [vp, u64, u64]; L.rwkv_state_copy.restype = i32
    for f in ("rwkv_score_rows", "rwkv_score"):
        getattr(L, f).argtypes = [vp, C.POINTER(u64), C.POINTER(u64), u64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(u64)]
        getattr(L, f).restype = i32
    npp = C.POINTER(NucleusParams)
    L.rwkv_sample_nucleus.argtypes = [vp, u64, u64, npp, C.c_double, C.POINTER(u64)]; L.rwkv_sample_nucleus.restype = i32
    L.rwkv_decode_nucleus.argtypes = [vp, u64, u64, npp, u64, C.POINTER(u64)]; L.rwkv_decode_nucleus.restype = i32
    L.rwkv_decode_batch_nucleus.argtypes = [vp, C.POINTER(u64), u64, u64, npp, C.POINTER(u64), C.POINTER(u64)]; L.rwkv_decode_batch_nucleus.restype = i32
    L.rwkv_penalty_set.argtypes = [vp, u64, vp]; L.rwkv_penalty_set.restype = i32
    L.rwkv_penalty_get.argtypes = [vp, u64, vp]; L.rwkv_penalty_get.restype = i32
    L.rwkv_decode_batch_until.argtypes = [vp, C.POINTER(u64), u64, u64, C.POINTER(Pick), C.POINTER(u64), C.POINTER(StopParams), C.POINTER(u64),
                                          C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(u64)]
    L.rwkv_decode_batch_until.restype = i32
    L.rwkv_debug_stop_scan.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), u64, u64, C.POINTER(StopParams), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.rwkv_debug_stop_scan.restype = i32
    L.rwkv_topn_rows.argtypes = [vp, C.POINTER(u64), u64, C.c_uint32, C.POINTER(u64), C.POINTER(C.c_double)]; L.rwkv_topn_rows.restype = i32
    L.rwkv_decode_batch_logprobs.argtypes = [vp, C.POINTER(u64), u64, u64, C.POINTER(Pick), C.POINTER(u64), C.POINTER(StopParams), C.POINTER(LogprobOut),
                                             C.POINTER(u64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(u64)]
    L.rwkv_decode_batch_logprobs.restype = i32
    L.rwkv_decode_beam.argtypes = [vp, u64, u64, C.POINTER(BeamParams), C.POINTER(BeamOut)]; L.rwkv_decode_beam.restype = i32
    L.rwkv_state_permute.argtypes = [vp, C.POINTER(C.c_uint32), u64]; L.rwkv_state_permute.restype = i32
    L.rwkv_debug_beam_step.argtypes = [vp, C.POINTER(BeamParams), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(u64), C.POINTER(C.c_uint32),
                                       C.POINTER(u64), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint8)]
    L.rwkv_debug_beam_step.restype = i32
    u32p = C.POINTER(C.c_uint32)
    L.rwkv_constraint_set.argtypes = [vp, C.POINTER(Automaton)]; L.rwkv_constraint_set.restype = i32
    L.rwkv_constraint_clear.argtypes = [vp]; L.rwkv_constraint_clear.restype = i32
    L.rwkv_constraint_state_set.argtypes = [vp, u64, u64, u32p]; L.rwkv_constraint_state_set.restype = i32
    L.rwkv_constraint_state_get.argtypes = [vp, u64, u64, u32p]; L.rwkv_constraint_state_get.restype = i32
    L.rwkv_pick_constrained.argtypes = [vp, u64, u64, C.POINTER(Pick), C.POINTER(Bias), C.c_double, i32, C.POINTER(u64), u32p]
    L.rwkv_pick_constrained.restype = i32
    L.rwkv_debug_constrained_row.argtypes = [vp, u64, vp]; L.rwkv_debug_constrained_row.restype = i32
    L.rwkv_decode_batch_constrained.argtypes = [vp, C.POINTER(u64), u64, u64, C.POINTER(Pick), C.POINTER(u64), C.POINTER(ConstrainParams),
                                                C.POINTER(StopParams), C.POINTER(LogprobOut), C.POINTER(u64), u32p, u32p, C.POINTER(u64)]
    L.rwkv_decode_batch_constrained.restype = i32
    L.rwkv_spec_verify.argtypes = [vp, u64, C.POINTER(u64), u64, C.POINTER(u64), C.POINTER(u64)]; L.rwkv_spec_verify.restype = i32
    L.rwkv_decode_speculative.argtypes = [vp, vp, u64, u64, C.c_uint32, C.POINTER(u64), C.POINTER(SpecStats)]; L.rwkv_decode_speculative.restype = i32
    L.rwkv_forward_segments.argtypes = [vp, C.POINTER(u64), C.POINTER(Segment), u64, C.c_uint32, C.POINTER(u64)]; L.rwkv_forward_segments.restype = i32
    L.rwkv_segment_plan.argtypes = [C.POINTER(Segment), u64, u64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(u64)]; L.rwkv_segment_plan.restype = i32
    _lib = L
    return L


def _chk(rc: int):
    if rc != 0:
        raise RWKVError(lib().rwkv_last_error().decode(errors="replace") + f" (status {rc})")


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class RWKVState:
    """Mirror of reference class RWKVState (rwkv.h:140-242): five host arrays [stateSize][L][D] f64."""

    def __init__(self, num_layers: int, num_embed: int, stateSize: int = 1):
        self.num_layers, self.num_embed, self.stateSize = num_layers, num_embed, stateSize
        n = num_layers * num_embed * stateSize
        self.statexy = np.zeros(n); self.stateaa = np.zeros(n); self.statebb = np.zeros(n)
        self.statepp = np.zeros(n); self.statedd = np.zeros(n)

    def arrays(self):
        return [self.statexy, self.stateaa, self.statebb, self.statepp, self.statedd]

    def copy(self) -> "RWKVState":
        s = RWKVState(self.num_layers, self.num_embed, self.stateSize)
        for d, a in zip(s.arrays(), self.arrays()):
            d[:] = a
        return s

    def getSubState(self, offset: int = 0) -> "RWKVState":                      # rwkv.h:223-228
        if offset >= self.stateSize:
            raise RuntimeError(f"State get offset out of bounds, max offset is {self.stateSize}")
        n = self.num_layers * self.num_embed
        s = RWKVState(self.num_layers, self.num_embed, 1)
        for d, a in zip(s.arrays(), self.arrays()):
            d[:] = a[offset * n:(offset + 1) * n]   # (the reference's ctor ignores the L*D stride, rwkv.h:205; fixed)
        return s

    def setSubState(self, other: "RWKVState", offset: int = 0):                 # rwkv.h:231-240
        n = self.num_layers * self.num_embed
        for d, a in zip(self.arrays(), other.arrays()):
            d[offset * n:(offset + 1) * n] = a[:n]


class RWKV:
    """Mirror of reference class RWKV (rwkv.h:245-429) on top of the C-ABI.

    Default semantics are the reference's: the HOST state is authoritative and is uploaded before
    / downloaded after every forward (rwkv.h:353,372).  `resident=True` keeps the state on the
    device between calls (sync explicitly with pull_state/push_state): the engine's fast path."""

    def __init__(self, device: int = 0, resident: bool = False):
        self._h = C.c_void_p()
        _chk(lib().rwkv_create(C.byref(self._h), device))
        self.ready = False
        self.resident = resident
        self.num_layers = self.num_embed = 0
        self.maxContext = 1
        self.state = None
        self.out = None

    # -- loading ---------------------------------------------------------------------------
    def _after_load(self):
        L = lib()
        self.num_layers = int(L.rwkv_n_layers(self._h)); self.num_embed = int(L.rwkv_n_embed(self._h))
        self.maxContext = int(L.rwkv_max_ctx(self._h))
        self.state = RWKVState(self.num_layers, self.num_embed, self.maxContext)
        self.out = np.zeros(mf.VOCAB * self.maxContext, dtype=np.float32)
        self.ready = True

    def loadFile(self, filename: str, maxGPT: int = 1):                          # rwkv.h:281-310
        if self.ready:
            raise RuntimeError("RWKV already loaded")
        _chk(lib().rwkv_load_file(self._h, os.fsencode(filename), maxGPT))
        self._after_load()

    def loadTensors(self, n_layers: int, n_embed: int, tensors, maxGPT: int = 1):
        """46 tensors in file layout: numpy arrays (host) or torch CUDA tensors (device), not mixed;
        scratch/state slots may be None."""
        if self.ready:
            raise RuntimeError("RWKV already loaded")
        ptrs = (C.c_void_p * mf.N_TENSORS)()
        on_device = None
        keep = []
        for i, t in enumerate(tensors):
            if t is None:
                if i not in mf.BUFFER_SLOTS:
                    raise ValueError(f"tensor {i} ({mf.NAMES[i]}) is required")
                ptrs[i] = None
                continue
            if isinstance(t, np.ndarray):
                a = np.ascontiguousarray(t, dtype=mf.DTYPES[i]); keep.append(a)
                ptrs[i] = a.ctypes.data; dev = False
            else:   # torch tensor
                tt = t.contiguous(); keep.append(tt)
                ptrs[i] = tt.data_ptr(); dev = tt.is_cuda
                if tt.numel() * tt.element_size() != mf.sizes(n_layers, n_embed)[i] * np.dtype(mf.DTYPES[i]).itemsize:
                    raise ValueError(f"tensor {i} ({mf.NAMES[i]}) has the wrong byte size")
            if i in mf.BUFFER_SLOTS:
                continue
            if on_device is None:
                on_device = dev
            elif on_device != dev:
                raise ValueError("tensors must be all host or all device")
        if on_device:
            import torch
            torch.cuda.synchronize()
        _chk(lib().rwkv_load_tensors(self._h, n_layers, n_embed, ptrs, 1 if on_device else 0, maxGPT))
        self._after_load()

    # -- layer pipeline ---------------------------------------------------------------------
    def set_layer_range(self, l0: int, l1: int):
        _chk(lib().rwkv_set_layer_range(self._h, l0, l1))

    def stage_forward(self, token: int, slot: int = 0, want_pick: bool = False):
        pick = C.c_uint64(0)
        _chk(lib().rwkv_stage_forward(self._h, int(token), slot, C.byref(pick) if want_pick else None))
        return int(pick.value) if want_pick else None

    def x_device_ptr(self) -> int:
        return int(lib().rwkv_x_device(self._h) or 0)

    def xseq_device_ptr(self, buf: int = 0) -> int:
        """device address of residual-stream buffer `buf` (0 / 1) of the chunk path: [rows][n_embed] f64, what stage_chunk reads and leaves"""
        return int(lib().rwkv_xseq_device(self._h, int(buf)) or 0)

    def stage_chunk(self, tokens, n: int, row0: int = 0, buf: int = 0):
        """one prompt chunk (n <= 32 tokens) through this stage's layers on the mm8_seq path (asynchronous)"""
        arr = (C.c_uint64 * n)(*[int(t) for t in tokens]) if tokens is not None else None
        _chk(lib().rwkv_stage_chunk(self._h, arr, n, row0, buf))

    def xseq_copy_from(self, src: "RWKV", rows: int, buf: int = 0):
        """same-device hand-over of a chunk's residual stream from the previous stage's context"""
        _chk(lib().rwkv_xseq_copy(self._h, buf, src._h, buf, rows))

    def sync(self):
        _chk(lib().rwkv_sync(self._h))

    # -- native pipeline transport (RCCL inside the engine) ------------------------------------
    @staticmethod
    def pipe_rccl_path() -> str:
        """the RCCL shared object the pipeline transport binds in this process (RWKV_RCCL_LIB, else the one already loaded -- torch's --, else the system's)"""
        buf = C.create_string_buffer(4096)
        _chk(lib().rwkv_pipe_rccl_path(buf, len(buf)))
        return buf.value.decode()

    @staticmethod
    def pipe_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        _chk(lib().rwkv_pipe_unique_id(buf))
        return buf.raw

    def pipe_init(self, unique_id: bytes, rank: int, world: int):
        assert len(unique_id) == 128
        _chk(lib().rwkv_pipe_init(self._h, C.create_string_buffer(unique_id, 128), rank, world))

    def pipe_info(self) -> dict:
        """this rank's end of the transport (rwkv_pipe_info): rank, world, layers, device, PCI bus id, arch, RCCL version + path, prefill rows"""
        import json
        buf = C.create_string_buffer(2048)
        _chk(lib().rwkv_pipe_info(self._h, buf, len(buf)))
        return json.loads(buf.value.decode())

    def pipe_decode(self, first_tokens, n_steps: int, world: int, last: bool, n_streams: int | None = None):
        """greedy decode of n_streams (default: world) streams over the stages; [world][n_steps] ids on the last rank"""
        ft = (C.c_uint64 * world)(*([int(t) for t in first_tokens] + [0] * world)[:world]) if first_tokens is not None else None
        picks = (C.c_uint64 * (world * n_steps))() if last else None
        _chk(lib().rwkv_pipe_decode_streams(self._h, ft, n_steps, world if n_streams is None else n_streams, picks))
        return np.frombuffer(picks, dtype=np.uint64).reshape(world, n_steps).astype(np.int64) if last else None

    def pipe_decode_dual(self, first_tokens, n_steps: int, world: int, last: bool):
        """greedy decode of 2 * world streams, two per stage in flight on two communicators (the hop of one under the stage of the other);
        [2 * world][n_steps] ids on the last rank"""
        n = 2 * world
        ft = (C.c_uint64 * n)(*([int(t) for t in first_tokens] + [0] * n)[:n]) if first_tokens is not None else None
        picks = (C.c_uint64 * (n * n_steps))() if last else None
        _chk(lib().rwkv_pipe_decode_dual(self._h, ft, n_steps, picks))
        return np.frombuffer(picks, dtype=np.uint64).reshape(n, n_steps).astype(np.int64) if last else None

    def pipe_profile(self, on: bool = True):
        _chk(lib().rwkv_pipe_profile(self._h, 1 if on else 0))

    def pipe_hop_stats(self):
        """{n, mean_us, min_us, max_us} of the event pairs around the per-tick RCCL group of the last pipe_decode"""
        out = (C.c_double * 4)()
        _chk(lib().rwkv_pipe_hop_stats(self._h, out))
        return dict(n=int(out[0]), mean_us=float(out[1]), min_us=float(out[2]), max_us=float(out[3]))

    def pipe_prefill(self, tokens, n_tokens: int):
        arr = (C.c_uint64 * n_tokens)(*[int(t) for t in tokens]) if tokens is not None else None
        _chk(lib().rwkv_pipe_prefill(self._h, arr, n_tokens))

    def tensor_device_ptr(self, slot: int) -> int:
        return int(lib().rwkv_tensor_device(self._h, slot) or 0)

    # -- state sync --------------------------------------------------------------------------
    def push_state(self, n_slots: int | None = None):
        n = self.maxContext if n_slots is None else n_slots
        _chk(lib().rwkv_set_state(self._h, *[_ptr(a) for a in self.state.arrays()], n))

    def pull_state(self, n_slots: int | None = None):
        n = self.maxContext if n_slots is None else n_slots
        _chk(lib().rwkv_get_output(self._h, None, *[_ptr(a) for a in self.state.arrays()], n))

    def reset_state(self):
        for a in self.state.arrays():
            a[:] = 0
        _chk(lib().rwkv_reset_state(self._h))

    # -- forward -----------------------------------------------------------------------------
    def forward(self, token, mode: int = MODE_GPT):                               # rwkv.h:339-388
        if not self.ready:
            raise RuntimeError("RWKV not loaded")
        toks = [int(token)] if np.isscalar(token) else [int(t) for t in token]
        if len(toks) > self.maxContext:
            raise RuntimeError(f"Context too large, max context is {self.maxContext}")
        T = len(toks)
        arr = (C.c_uint64 * T)(*toks)
        if not self.resident:
            self.push_state(T)                                                    # setState, rwkv.h:353
        _chk(lib().rwkv_forward(self._h, arr, T, mode))
        if self.resident:
            _chk(lib().rwkv_get_output(self._h, _ptr(self.out), None, None, None, None, None, T))
        else:
            _chk(lib().rwkv_get_output(self._h, _ptr(self.out), *[_ptr(a) for a in self.state.arrays()], T))   # rwkv.h:372
        return self.out

    def decode_greedy(self, first_token: int, n_tokens: int) -> np.ndarray:
        """device-side greedy continuation on the resident state (slot 0); returns the picked ids."""
        if not self.ready:
            raise RuntimeError("RWKV not loaded")
        out = (C.c_uint64 * n_tokens)()
        if not self.resident:
            self.push_state(1)          # host state is authoritative: continue from it ...
        _chk(lib().rwkv_decode_greedy(self._h, int(first_token), n_tokens, out))
        if not self.resident:
            self.pull_state(1)          # ... and leave it where the generated tokens ended
        return np.frombuffer(out, dtype=np.uint64).copy()

    def sample_typical(self, temp: float = 0.9, tau: float = 0.8, u: float = 0.5, row: int = 0, ban0: bool = False, recipe: bool = False) -> int:
        """the reference's typical() ON THE DEVICE from the logits of the last forward (reference typical.h:20-58); u in
        [0, 1) is the caller's uniform -- the draw is the inverse CDF in token order.  Default: what the reference computes,
        a draw from softmax^(1/temp) (its cut at tau is a no-op, typical.h:50); recipe=True applies the documented cut."""
        tok = C.c_uint64(0)
        flags = (SAMPLE_BAN0 if ban0 else 0) | (SAMPLE_RECIPE if recipe else 0)
        _chk(lib().rwkv_sample_typical(self._h, int(row), float(temp), float(tau), float(u), flags, C.byref(tok)))
        return int(tok.value)

    def decode_typical(self, first_token: int, n_tokens: int, temp: float = 0.9, tau: float = 0.8, seed: int = 0, recipe: bool = False) -> np.ndarray:
        """device-side sampled continuation (storygen's loop with the device sampler; logit 0 banned)"""
        out = (C.c_uint64 * n_tokens)()
        if not self.resident:
            self.push_state(1)
        _chk(lib().rwkv_decode_typical(self._h, int(first_token), n_tokens, float(temp), float(tau), int(seed),
                                       SAMPLE_RECIPE if recipe else 0, out))
        if not self.resident:
            self.pull_state(1)
        return np.frombuffer(out, dtype=np.uint64).copy()

    # -- batched decode: N streams on state slots 0 .. N - 1 ------------------------------------
    def _decode_batch(self, first_tokens, n_steps: int, call):
        if not self.ready:
            raise RuntimeError("RWKV not loaded")
        ft = [int(t) for t in first_tokens]
        n = len(ft)
        out = (C.c_uint64 * max(1, n * n_steps))()
        if not self.resident and 0 < n <= self.maxContext:
            self.push_state(n)          # host state is authoritative: continue the N slots from it ...
        _chk(call((C.c_uint64 * max(1, n))(*ft), n, out))
        if not self.resident:
            self.pull_state(n)          # ... and leave them where the generated tokens ended
        return np.frombuffer(out, dtype=np.uint64)[: n * n_steps].reshape(n, n_steps).copy()

    def decode_batch_greedy(self, first_tokens, n_steps: int) -> np.ndarray:
        """device-side greedy continuation of len(first_tokens) independent streams (stream s on state slot s, logit 0 banned);
        returns the picked ids [N][n_steps]"""
        return self._decode_batch(first_tokens, n_steps, lambda ft, n, out: lib().rwkv_decode_batch_greedy(self._h, ft, n, n_steps, out))

    def decode_batch_typical(self, first_tokens, n_steps: int, temp: float = 0.9, tau: float = 0.8, seeds=None, recipe: bool = False) -> np.ndarray:
        """the same with the device sampler: stream s draws what decode_typical(seed=seeds[s]) draws (default seeds: 0 .. N - 1)"""
        sd = list(range(len(first_tokens))) if seeds is None else [int(x) for x in seeds]
        if len(sd) != len(first_tokens):
            raise ValueError("need one seed per stream")
        arr = (C.c_uint64 * max(1, len(sd)))(*sd)
        return self._decode_batch(first_tokens, n_steps, lambda ft, n, out: lib().rwkv_decode_batch_typical(
            self._h, ft, n, n_steps, float(temp), float(tau), arr, SAMPLE_RECIPE if recipe else 0, out))

    # -- nucleus sampling with repetition penalties (include/rwkv_mi355x.h rwkv_sample_nucleus) --------
    def sample_nucleus(self, temp: float = 1.0, top_p: float = 0.9, top_k: int = 0, presence: float = 0.0, frequency: float = 0.0,
                       decay: float = 1.0, u: float = 0.5, row: int = 0, slot: int = 0, ban0: bool = False, update: bool = False) -> int:
        """temperature / top-p / top-k draw ON THE DEVICE from logits row `row` of the last forward, penalised by the occurrence counts of
        state slot `slot`; u in [0, 1) is the caller's uniform; update=True counts the pick (counts * decay, then + 1)"""
        tok = C.c_uint64(0)
        p = nucleus_params(temp, top_p, top_k, presence, frequency, decay, (NUCLEUS_BAN0 if ban0 else 0) | (NUCLEUS_UPDATE if update else 0))
        _chk(lib().rwkv_sample_nucleus(self._h, int(row), int(slot), C.byref(p), float(u), C.byref(tok)))
        return int(tok.value)

    def decode_nucleus(self, first_token: int, n_tokens: int, temp: float = 1.0, top_p: float = 0.9, top_k: int = 0, presence: float = 0.0,
                       frequency: float = 0.0, decay: float = 1.0, seed: int = 0, keep: bool = False) -> np.ndarray:
        """device-side sampled continuation on slot 0 with the nucleus sampler (logit 0 banned, counts updated every step; keep=False
        starts from zero counts)"""
        out = (C.c_uint64 * n_tokens)()
        p = nucleus_params(temp, top_p, top_k, presence, frequency, decay, NUCLEUS_KEEP if keep else 0)
        if not self.resident:
            self.push_state(1)
        _chk(lib().rwkv_decode_nucleus(self._h, int(first_token), n_tokens, C.byref(p), int(seed), out))
        if not self.resident:
            self.pull_state(1)
        return np.frombuffer(out, dtype=np.uint64).copy()

    def decode_batch_nucleus(self, first_tokens, n_steps: int, temp: float = 1.0, top_p: float = 0.9, top_k: int = 0, presence: float = 0.0,
                             frequency: float = 0.0, decay: float = 1.0, seeds=None, keep: bool = False) -> np.ndarray:
        """the same for len(first_tokens) streams: stream s on slot s draws what decode_nucleus(seed=seeds[s]) draws (default seeds: 0 .. N - 1)"""
        sd = list(range(len(first_tokens))) if seeds is None else [int(x) for x in seeds]
        if len(sd) != len(first_tokens):
            raise ValueError("need one seed per stream")
        arr = (C.c_uint64 * max(1, len(sd)))(*sd)
        p = nucleus_params(temp, top_p, top_k, presence, frequency, decay, NUCLEUS_KEEP if keep else 0)
        return self._decode_batch(first_tokens, n_steps, lambda ft, n, out: lib().rwkv_decode_batch_nucleus(
            self._h, ft, n, n_steps, C.byref(p), arr, out))

    # -- stop sequences and per-stream budgets in the device loops (include/rwkv_mi355x.h rwkv_decode_batch_until) --------
    def decode_batch_until(self, first_tokens, n_steps: int, stops=(), max_new=None, keep: bool = False, pick: str = "greedy", seeds=None,
                           temp: float = 1.0, tau: float = 0.8, recipe: bool = False, top_p: float = 0.9, top_k: int = 0, presence: float = 0.0,
                           frequency: float = 0.0, decay: float = 1.0, _logprobs=None, _constrain=None):
        """decode_batch_greedy / _typical / _nucleus (pick = "greedy", "typical", "nucleus", with that call's parameters) in which stream s ends
        at the first of the stop sequences `stops` (lists of token ids, each 1 .. 8 long) that its newest ids spell, or after max_new[s] tokens.
        keep: the match history (and the nucleus counts) continue from the previous call.  Returns (ids [N][n_steps], 0 behind a stream's end;
        len [N]; reason [N]: 0 ran all n_steps, 1 budget, 2 + j matched stops[j]; steps_run).  Slot s is left as it was when stream s stopped:
        feed ids[s][len[s] - 1] to continue it."""
        kind = {"greedy": PICK_GREEDY, "typical": PICK_TYPICAL, "nucleus": PICK_NUCLEUS}[pick]
        n = len(first_tokens)
        sd = list(range(n)) if seeds is None else [int(x) for x in seeds]
        if len(sd) != n:
            raise ValueError("need one seed per stream")
        if max_new is not None and len(max_new) != n:
            raise ValueError("need one budget per stream")
        arr = (C.c_uint64 * max(1, n))(*sd)
        pk = Pick(kind, float(temp), float(tau), SAMPLE_RECIPE if recipe else 0,
                  nucleus_params(temp, top_p, top_k, presence, frequency, decay, NUCLEUS_KEEP if keep else 0))
        sp, alive = stop_params(stops, max_new, keep)
        ln, rs, ran = (C.c_uint32 * max(1, n))(), (C.c_uint32 * max(1, n))(), C.c_uint64(0)
        sdp = None if kind == PICK_GREEDY else arr
        if _constrain is not None:      # decode_batch_constrained: the same call with the constraint hook (and the record, or none)
            call = lambda ft, n_, out: lib().rwkv_decode_batch_constrained(self._h, ft, n_, n_steps, C.byref(pk), sdp, C.byref(_constrain), C.byref(sp),
                                                                           None if _logprobs is None else C.byref(_logprobs), out, ln, rs, C.byref(ran))
        elif _logprobs is None:
            call = lambda ft, n_, out: lib().rwkv_decode_batch_until(self._h, ft, n_, n_steps, C.byref(pk), sdp, C.byref(sp), out, ln, rs, C.byref(ran))
        else:       # decode_batch_logprobs: the same call with the record
            call = lambda ft, n_, out: lib().rwkv_decode_batch_logprobs(self._h, ft, n_, n_steps, C.byref(pk), sdp, C.byref(sp), C.byref(_logprobs),
                                                                        out, ln, rs, C.byref(ran))
        ids = self._decode_batch(first_tokens, n_steps, call)
        del alive
        return (ids, np.frombuffer(ln, dtype=np.uint32)[:n].astype(np.int64), np.frombuffer(rs, dtype=np.uint32)[:n].astype(np.int64), int(ran.value))

    # -- log-probs and top-n alternatives of generated tokens (include/rwkv_mi355x.h rwkv_decode_batch_logprobs) --------
    def decode_batch_logprobs(self, first_tokens, n_steps: int, top_n: int = 0, entropy: bool = True, **kw):
        """decode_batch_until (its arguments: stops, max_new, keep, pick, seeds and the pick's parameters) that also returns what the MODEL thought
        of every generated token -- no penalty, no temperature, nothing banned, whichever pick generated it.  Returns (ids, len, reason,
        steps_run, logprob [N][n_steps], entropy [N][n_steps] or None, top_ids [N][n_steps][top_n], top_logprob likewise); every entry behind a
        stream's end is 0 / 0.0.  Best-of-n: rank streams by logprob[s, :len[s]].sum()."""
        n, e = len(first_tokens), max(1, len(first_tokens) * int(n_steps))
        top_n = int(top_n)
        lp, ent = np.zeros(e, dtype=np.float64), (np.zeros(e, dtype=np.float64) if entropy else None)
        tid, tlp = np.zeros(e * max(1, top_n), dtype=np.uint64), np.zeros(e * max(1, top_n), dtype=np.float64)
        dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
        rec = LogprobOut(top_n, 0, lp.ctypes.data_as(dp), ent.ctypes.data_as(dp) if entropy else None,
                         tid.ctypes.data_as(up) if top_n > 0 else None, tlp.ctypes.data_as(dp) if top_n > 0 else None)
        ids, ln, rs, ran = self.decode_batch_until(first_tokens, n_steps, _logprobs=rec, **kw)
        shape = (n, int(n_steps))
        return (ids, ln, rs, ran, lp[: n * n_steps].reshape(shape), ent[: n * n_steps].reshape(shape) if entropy else None,
                tid[: n * n_steps * top_n].astype(np.int64).reshape(shape + (top_n,)), tlp[: n * n_steps * top_n].reshape(shape + (top_n,)))

    # -- constrained decoding: a token automaton and a logit bias (include/rwkv_mi355x.h rwkv_decode_batch_constrained) --------
    def constraint_set(self, row_ptr, tok, next):
        """install the token-level automaton (row_ptr [S + 1], tok [nnz], next [nnz], u32; a state without edges is terminal) -- what a regex,
        grammar or choice-list compiler of the caller's produced, or constraint_trie(choices).  Every slot's automaton state becomes 0."""
        rp, tk, nx = (np.ascontiguousarray(a, dtype=np.uint32) for a in (row_ptr, tok, next))
        if rp.size < 1 or tk.size != nx.size:
            raise ValueError("row_ptr has S + 1 entries, tok and next nnz each")
        u32p = C.POINTER(C.c_uint32)
        a = Automaton(rp.size - 1, 0, tk.size, rp.ctypes.data_as(u32p), tk.ctypes.data_as(u32p) if tk.size else None,
                      nx.ctypes.data_as(u32p) if nx.size else None)
        _chk(lib().rwkv_constraint_set(self._h, C.byref(a)))

    def constraint_clear(self):
        _chk(lib().rwkv_constraint_clear(self._h))

    def constraint_state_get(self, slot0: int = 0, n: int | None = None) -> np.ndarray:
        """the automaton states of slots slot0 .. slot0 + n - 1 (default: all)"""
        n = self.maxContext - int(slot0) if n is None else int(n)
        out = np.zeros(max(1, n), dtype=np.uint32)
        _chk(lib().rwkv_constraint_state_get(self._h, int(slot0), n, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out[:n].astype(np.int64)

    def constraint_state_set(self, states, slot0: int = 0):
        a = np.ascontiguousarray([int(v) for v in states], dtype=np.uint32)
        _chk(lib().rwkv_constraint_state_set(self._h, int(slot0), a.size, a.ctypes.data_as(C.POINTER(C.c_uint32))))

    def pick_constrained(self, pick: str = "greedy", bias=None, u: float = 0.5, advance: bool = True, row: int = 0, slot: int = 0, temp: float = 1.0,
                         top_p: float = 0.9, top_k: int = 0, presence: float = 0.0, frequency: float = 0.0, decay: float = 1.0, update: bool = False):
        """ONE constrained draw from logits row `row` of the last forward under the automaton state of slot `slot` and the bias list `bias`
        ({id: value}; -inf bans), greedy or nucleus with that call's parameters; advance: the slot's state moves along the pick.  Returns
        (token, the slot's automaton state on return).  Logits and state stay as they are."""
        kind = {"greedy": PICK_GREEDY, "typical": PICK_TYPICAL, "nucleus": PICK_NUCLEUS}[pick]
        pk = Pick(kind, float(temp), 0.8, 0, nucleus_params(temp, top_p, top_k, presence, frequency, decay, NUCLEUS_UPDATE if update else 0))
        b, alive = None, None
        if bias is not None:
            alive = _bias_arrays(bias)
            b = Bias(alive[0].size, 0, alive[0].ctypes.data_as(C.POINTER(C.c_uint32)), alive[1].ctypes.data_as(C.POINTER(C.c_float)))
        tok, q = C.c_uint64(0), C.c_uint32(0)
        _chk(lib().rwkv_pick_constrained(self._h, int(row), int(slot), C.byref(pk), None if b is None else C.byref(b), float(u), 1 if advance else 0,
                                         C.byref(tok), C.byref(q)))
        del alive
        return int(tok.value), int(q.value)

    def debug_constrained_row(self, row: int = 0) -> np.ndarray:
        """row `row` of the second buffer as the last constrained pick or step left it (float32 [50277])"""
        out = np.zeros(mf.VOCAB, dtype=np.float32)
        _chk(lib().rwkv_debug_constrained_row(self._h, int(row), _ptr(out)))
        return out

    def decode_batch_constrained(self, first_tokens, n_steps: int, start=None, bias=None, logprobs: bool = False, top_n: int = 0, **kw):
        """decode_batch_until (its arguments: stops, max_new, keep, pick = "greedy" or "nucleus", seeds and the pick's parameters) under the installed
        automaton and per-stream logit bias: stream s starts in automaton state start[s] (None: where slot s stands) with the bias list bias[s]
        ({id: value}, -inf bans; None: no bias) and also ends where its automaton reaches a terminal state (reason STOP_CONSTRAINT = 32).  Returns
        (ids, len, reason, steps_run, state [N]: the automaton state after the stream's len tokens); logprobs=True appends decode_batch_logprobs'
        logprob, entropy, top_ids, top_logprob -- the MODEL's, nothing of the mask shows in them."""
        n = len(first_tokens)
        u32p = C.POINTER(C.c_uint32)
        st = None if start is None else np.ascontiguousarray([int(v) for v in start], dtype=np.uint32)
        if st is not None and st.size != n:
            raise ValueError("need one start state per stream")
        bp = bt = bv = None
        if bias is not None:
            if len(bias) != n:
                raise ValueError("need one bias list per stream (an empty one for none)")
            lists = [_bias_arrays(b if b is not None else {}) for b in bias]
            bp = np.concatenate([[0], np.cumsum([t.size for t, _ in lists])]).astype(np.uint32)
            bt = np.concatenate([t for t, _ in lists] + [np.zeros(1, np.uint32)])          # (one entry of padding: the arrays are there when every list is empty)
            bv = np.concatenate([v for _, v in lists] + [np.zeros(1, np.float32)])
        out_state = np.zeros(max(1, n), dtype=np.uint32)
        cp = ConstrainParams(None if st is None else st.ctypes.data_as(u32p), None if bp is None else bp.ctypes.data_as(u32p),
                             None if bt is None else bt.ctypes.data_as(u32p), None if bv is None else bv.ctypes.data_as(C.POINTER(C.c_float)),
                             out_state.ctypes.data_as(u32p), 0)
        if logprobs:
            r = self.decode_batch_logprobs(first_tokens, n_steps, top_n=top_n, _constrain=cp, **kw)
        else:
            r = self.decode_batch_until(first_tokens, n_steps, _constrain=cp, **kw)
        return r[:4] + (out_state[:n].astype(np.int64),) + r[4:]

    def topn_rows(self, rows, top_n: int):
        """(ids [n][top_n], logprob [n][top_n]): the top_n most probable tokens of logits row rows[i] of the LAST forward (rwkv_topn_rows), in
        descending logit order, equal logits by ascending id; the log-probs are bit for bit those of score_rows.  Logits and state stay."""
        if not self.ready:
            raise RuntimeError("RWKV not loaded")
        r = [int(v) for v in rows]
        n, top_n = len(r), int(top_n)
        ids, lp = np.zeros(max(1, n * max(0, top_n)), dtype=np.uint64), np.zeros(max(1, n * max(0, top_n)), dtype=np.float64)
        _chk(lib().rwkv_topn_rows(self._h, (C.c_uint64 * max(1, n))(*r), n, top_n, ids.ctypes.data_as(C.POINTER(C.c_uint64)),
                                  lp.ctypes.data_as(C.POINTER(C.c_double))))
        return ids[: n * top_n].astype(np.int64).reshape(n, top_n), lp[: n * top_n].reshape(n, top_n)

    # -- beam search on the device (include/rwkv_mi355x.h rwkv_decode_beam) ---------------------------------------------------
    def decode_beam(self, first_token: int, n_steps: int, width: int = 4, stops=()):
        """the `width` most probable continuations of the prompt whose state slot 0 holds, fed first_token, n_steps long; stops: single-token stop
        ids that end a hypothesis.  Returns (tokens [W][n_steps], 0 behind a hypothesis's end; len [W]; score [W], the sum of the token
        log-probs; token_logprob [W][n_steps]); hypothesis 0 is the best.  Slot m is left where live hypothesis m ended: feed
        tokens[m][len[m] - 1] to go on.  A length penalty is the caller's: rank by score / len ** a."""
        if not self.ready:
            raise RuntimeError("RWKV not loaded")
        W, n = int(width), int(n_steps)
        e = max(1, W * n)
        tok, lp = np.zeros(e, dtype=np.uint64), np.zeros(e, dtype=np.float64)
        ln, sc = np.zeros(max(1, W), dtype=np.uint32), np.zeros(max(1, W), dtype=np.float64)
        bp, alive = beam_params(W, stops)
        out = BeamOut(tok.ctypes.data_as(C.POINTER(C.c_uint64)), ln.ctypes.data_as(C.POINTER(C.c_uint32)), sc.ctypes.data_as(C.POINTER(C.c_double)),
                      lp.ctypes.data_as(C.POINTER(C.c_double)))
        if not self.resident:
            self.push_state(1)          # host state is authoritative: the prompt's state is its slot 0 ...
        _chk(lib().rwkv_decode_beam(self._h, int(first_token), n, C.byref(bp), C.byref(out)))
        if not self.resident:
            self.pull_state(W)          # ... and every slot is left where its hypothesis ended
        del alive
        return tok[: W * n].astype(np.int64).reshape(W, n), ln[:W].astype(np.int64), sc[:W].copy(), lp[: W * n].reshape(W, n)

    def state_permute(self, parents):
        """slot m <- what slot parents[m] held, for every m < len(parents) at once (rwkv_state_permute; any map: swaps, cycles, fan-out); the
        other slots and the logits stay.  Re-fork the survivors of a best-of-n: state_permute([best, best, second, second])."""
        if not self.ready:
            raise RuntimeError("RWKV not loaded")
        p = [int(v) for v in parents]
        _chk(lib().rwkv_state_permute(self._h, (C.c_uint32 * max(1, len(p)))(*p), len(p)))
        if not self.resident:           # the host copy is the authoritative one
            n = self.num_layers * self.num_embed
            for a in self.state.arrays():
                old = a.copy()
                for m, q in enumerate(p):
                    a[m * n:(m + 1) * n] = old[q * n:(q + 1) * n]

    def debug_beam_step(self, cum, ended, last, stops=()):
        """ONE selection and state gather on whatever logits rows 0 .. W - 1 and the state slots hold (rwkv_debug_beam_step), W = len(cum):
        (parent [W], token [W], score [W], token_logprob [W], ended [W])"""
        c = np.ascontiguousarray(cum, dtype=np.float64)
        W = c.size
        e = np.ascontiguousarray([1 if v else 0 for v in ended], dtype=np.uint8)
        l = np.ascontiguousarray([int(v) for v in last], dtype=np.uint64)
        if e.size != W or l.size != W:
            raise ValueError("cum, ended and last have one entry per beam")
        bp, alive = beam_params(W, stops)
        par, tok = np.zeros(max(1, W), dtype=np.uint32), np.zeros(max(1, W), dtype=np.uint64)
        sc, lp, eo = np.zeros(max(1, W), dtype=np.float64), np.zeros(max(1, W), dtype=np.float64), np.zeros(max(1, W), dtype=np.uint8)
        dp = C.POINTER(C.c_double)
        _chk(lib().rwkv_debug_beam_step(self._h, C.byref(bp), c.ctypes.data_as(dp), e.ctypes.data_as(C.POINTER(C.c_uint8)),
                                        l.ctypes.data_as(C.POINTER(C.c_uint64)), par.ctypes.data_as(C.POINTER(C.c_uint32)),
                                        tok.ctypes.data_as(C.POINTER(C.c_uint64)), sc.ctypes.data_as(dp), lp.ctypes.data_as(dp),
                                        eo.ctypes.data_as(C.POINTER(C.c_uint8))))
        del alive
        return par[:W].astype(np.int64), tok[:W].astype(np.int64), sc[:W].copy(), lp[:W].copy(), eo[:W].astype(np.int64)

    # -- speculative greedy decoding (include/rwkv_mi355x.h rwkv_spec_verify) ---------------------------------------------------
    def spec_verify(self, token: int, draft=()):
        """feed [token, *draft] to slot 0 in ONE pass of the chunk path and keep the longest prefix of the draft that the greedy picks confirm:
        (n_accepted, next).  Slot 0 is left after token, draft[:n_accepted]; `next` is emitted and not fed.  len(draft) <= 31; an empty draft is a
        plain one-token step on the chunk path."""
        if not self.ready:
            raise RuntimeError("RWKV not loaded")
        d = [int(t) for t in draft]
        arr = (C.c_uint64 * max(1, len(d)))(*d)
        a, nx = C.c_uint64(0), C.c_uint64(0)
        if not self.resident:
            self.push_state(1)
        _chk(lib().rwkv_spec_verify(self._h, int(token), arr if d else None, len(d), C.byref(a), C.byref(nx)))
        if not self.resident:
            self.pull_state(1)
        return int(a.value), int(nx.value)

    # -- segmented forward (include/rwkv_mi355x.h rwkv_forward_segments) --------------------------------------------------------
    def forward_segments(self, segments):
        """one call of the chunk path over `segments`, a list of (slot, token_ids) with pairwise distinct slots: each sequence continues from its
        slot and leaves it after its ids, all behind one read of the weights per pass.  Row j of the logits buffer belongs to token j of the
        ids back to back; returns last_row, the row of each segment's last token (read it with logits / score_rows / topn_rows)."""
        if not self.ready:
            raise RuntimeError("RWKV not loaded")
        arr, n, ids = _segments(segments)
        toks = (C.c_uint64 * max(1, len(ids)))(*ids)
        last = (C.c_uint64 * max(1, n))()
        slots = min(self.maxContext, 1 + max([int(s.slot) for s in arr[:n]], default=0))
        if not self.resident:
            self.push_state(slots)
        _chk(lib().rwkv_forward_segments(self._h, toks, arr, n, 0, last))
        if not self.resident:
            self.pull_state(slots)
        return [int(r) for r in last[:n]]

    def decode_speculative(self, draft_model: "RWKV", first_token: int, n_tokens: int, k: int = 4):
        """greedy continuation of n_tokens ids with `draft_model` (a second loaded model on the same device whose slot 0 holds the same prefix,
        loaded with maxGPT >= k + 2) guessing k ids per round and this model verifying them in one pass: (ids, stats) with stats = dict(rounds,
        drafted, accepted).  The ids do not depend on the draft model.  Both models are left behind first_token, ids[:-1]."""
        if not self.ready or not draft_model.ready:
            raise RuntimeError("RWKV not loaded")
        n = int(n_tokens)
        out = (C.c_uint64 * max(1, n))()
        st = SpecStats()
        for m in (self, draft_model):
            if not m.resident:
                m.push_state(1)
        _chk(lib().rwkv_decode_speculative(self._h, draft_model._h, int(first_token), n, int(k), out, C.byref(st)))
        for m in (self, draft_model):
            if not m.resident:
                m.pull_state(1)
        return np.frombuffer(out, dtype=np.uint64)[:n].astype(np.int64), dict(rounds=int(st.rounds), drafted=int(st.drafted), accepted=int(st.accepted))

    def decode_lookup(self, history, n_tokens: int, k: int = 8, n: int = 3):
        """greedy continuation of n_tokens ids with the host-side lookup drafter (ngram_draft) in place of a draft model: history = the ids so
        far, of which all but the last have been fed (the last one is fed first).  Returns (ids, stats) like decode_speculative; the ids are
        those of repeated spec_verify(token, ())."""
        h = [int(t) for t in history]
        if not h:
            raise ValueError("history holds at least the id to feed first")
        n_tokens = int(n_tokens)
        out = []
        stats = dict(rounds=0, drafted=0, accepted=0)
        while len(out) < n_tokens:
            kd = min(int(k), SPEC_MAX_DRAFT, self.maxContext - 1, n_tokens - len(out) - 1)
            d = ngram_draft(h, kd, n) if kd > 0 else []
            a, nx = self.spec_verify(h[-1], d)
            new = d[:a] + [nx]
            out += new; h += new
            stats["rounds"] += 1; stats["drafted"] += len(d); stats["accepted"] += a
        return np.asarray(out, dtype=np.int64), stats

    def debug_stop_scan(self, ids, first_tokens, stops=(), max_new=None, keep: bool = False):
        """the stop test alone over PLANTED picks ids [n][steps] (rwkv_debug_stop_scan): (len [n], reason [n]); stream s uses slot s's history"""
        a = np.ascontiguousarray(ids, dtype=np.uint64)
        n, steps = a.shape
        ft = (C.c_uint64 * max(1, n))(*[int(t) for t in first_tokens])
        sp, alive = stop_params(stops, max_new, keep)
        ln, rs = (C.c_uint32 * max(1, n))(), (C.c_uint32 * max(1, n))()
        _chk(lib().rwkv_debug_stop_scan(self._h, a.ctypes.data_as(C.POINTER(C.c_uint64)), ft, n, steps, C.byref(sp), ln, rs))
        del alive
        return np.frombuffer(ln, dtype=np.uint32)[:n].astype(np.int64), np.frombuffer(rs, dtype=np.uint32)[:n].astype(np.int64)

    def penalty_set(self, slot: int, counts=None):
        """upload the occurrence counts of state slot `slot` (float32 [50277]; None: zero them)"""
        a = None if counts is None else np.ascontiguousarray(counts, dtype=np.float32)
        if a is not None and a.shape != (mf.VOCAB,):
            raise ValueError(f"counts must have shape ({mf.VOCAB},)")
        _chk(lib().rwkv_penalty_set(self._h, int(slot), _ptr(a)))

    def penalty_get(self, slot: int) -> np.ndarray:
        """the occurrence counts of state slot `slot` (float32 [50277])"""
        out = np.zeros(mf.VOCAB, dtype=np.float32)
        _chk(lib().rwkv_penalty_get(self._h, int(slot), _ptr(out)))
        return out

    def copy_state(self, dst: int, src: int):
        """copy state slot src into slot dst (fork a prefilled prompt into the slots of a batched decode)"""
        if not self.ready:
            raise RuntimeError("RWKV not loaded")
        _chk(lib().rwkv_state_copy(self._h, int(dst), int(src)))
        if not self.resident:           # the host copy is the authoritative one
            n = self.num_layers * self.num_embed
            for a in self.state.arrays():
                a[dst * n:(dst + 1) * n] = a[src * n:(src + 1) * n]

    # -- scoring: log-probability, entropy and argmax per logits row, on the device --------------
    def _score(self, call, first, targets):
        a, g = [int(v) for v in first], [int(v) for v in targets]
        if len(a) != len(g):
            raise ValueError("need one target per query")
        n = len(a)
        lp, ent, am = (C.c_double * max(1, n))(), (C.c_double * max(1, n))(), (C.c_uint64 * max(1, n))()
        _chk(call(self._h, (C.c_uint64 * max(1, n))(*a), (C.c_uint64 * max(1, n))(*g), n, lp, ent, am))
        return (np.frombuffer(lp, dtype=np.float64)[:n].copy(), np.frombuffer(ent, dtype=np.float64)[:n].copy(),
                np.frombuffer(am, dtype=np.uint64)[:n].astype(np.int64))

    def score_rows(self, rows, targets):
        """(logprob, entropy, argmax) of targets[i] under logits row rows[i] of the LAST forward (rwkv_score_rows): f64 log-softmax,
        entropy in nats and the lowest id of the largest logit, computed on the device; logits and state stay as they are"""
        if not self.ready:
            raise RuntimeError("RWKV not loaded")
        return self._score(lib().rwkv_score_rows, rows, targets)

    def score(self, tokens, targets=None):
        """feed `tokens` in GPT mode on slot 0 from the current state and score targets[t] under the logits that follow tokens[t]
        (rwkv_score; any length, in pieces of maxContext tokens as a loop of forward() would run them).  targets=None scores a document:
        tokens[:-1] are fed against tokens[1:].  Returns (logprob, entropy, argmax)."""
        if not self.ready:
            raise RuntimeError("RWKV not loaded")
        toks = [int(t) for t in tokens]
        if targets is None:
            toks, targets = toks[:-1], toks[1:]
        if not self.resident:
            self.push_state(1)          # host state is authoritative: continue from it ...
        out = self._score(lib().rwkv_score, toks, targets)
        if not self.resident:
            self.pull_state(1)          # ... and leave it where the scored tokens ended
        return out

    def logits(self, n_tokens: int = 1) -> np.ndarray:
        _chk(lib().rwkv_get_output(self._h, _ptr(self.out), None, None, None, None, None, n_tokens))
        return self.out[: n_tokens * mf.VOCAB]

    def emptyState(self) -> RWKVState:                                            # rwkv.h:390-393
        return RWKVState(self.num_layers, self.num_embed, 1)

    def getTensorSize(self, i: int) -> int:                                       # rwkv.h:325-328
        return mf.sizes(self.num_layers, self.num_embed)[i]

    def getTensorTypes(self, i: int) -> int:                                      # rwkv.h:331-334
        return np.dtype(mf.DTYPES[i]).itemsize

    # -- measurement -------------------------------------------------------------------------
    def bytes_per_token(self) -> int:
        return int(lib().rwkv_bytes_per_token(self._h))

    def profile_token(self, token: int = 1, reps: int = 8):
        ms = (C.c_double * N_KCLASS)(); by = (C.c_uint64 * N_KCLASS)(); ln = (C.c_uint32 * N_KCLASS)()
        _chk(lib().rwkv_profile_token(self._h, token, reps, ms, by, ln))
        return [dict(name=KCLASS_NAMES[k], ms_total=ms[k], reps=reps, launches_per_token=int(ln[k]),
                     bytes_per_launch=int(by[k])) for k in range(N_KCLASS)]

    def profile_batched(self, token: int = 1, reps: int = 4):
        """per-class launch duration from one event pair around reps x L back-to-back launches (resets the state)"""
        ms = (C.c_double * N_KCLASS)(); n = (C.c_uint32 * N_KCLASS)()
        _chk(lib().rwkv_profile_batched(self._h, token, reps, ms, n))
        by = [p["bytes_per_launch"] for p in self.profile_token(token, 1)]
        return [dict(name=KCLASS_NAMES[k], us=1e3 * ms[k] / max(1, n[k]), launches=int(n[k]), bytes_per_launch=by[k]) for k in range(N_KCLASS)]

    def debug_timeline(self, token: int = 1, grid: int = 256):
        buf = np.zeros(512 * 8 * 8, dtype=np.uint64)
        _chk(lib().rwkv_debug_timeline(self._h, token, _ptr(buf), buf.size))
        return buf

    def resident_bytes(self) -> int:
        return int(lib().rwkv_resident_bytes(self._h))

    def decode_form(self) -> int:
        """Mask of the per-layer decode kernel classes that stream the tile image (bit 0 K/V/R, 1 att_out, 2 ffn k/r, 3 ffn_v)."""
        return int(lib().rwkv_decode_form(self._h))

    # ---- per-kernel parity hooks (include/rwkv_mi355x.h rwkv_debug_launch): the production decode kernels one launch at a time ----
    DBG = dict(x=(0, np.float64), ybuf=(1, np.float32), part_att=(2, np.float64), pmax_att=(3, np.float32), hbuf=(4, np.float32),
               rgate=(5, np.float32), part_ffn=(6, np.float64), pmax_ffn=(7, np.float32), lnstat=(8, np.float64))

    def debug_launch(self, cls, layer=0, token=0, slot=0):
        _chk(lib().rwkv_debug_launch(self._h, int(cls), int(layer), int(token), int(slot)))

    def debug_grid(self):
        return int(lib().rwkv_debug_grid(self._h))

    def debug_read(self, name):
        which, dt = self.DBG[name]
        D, G = self.num_embed, self.debug_grid()
        n = dict(x=D, ybuf=D, part_att=G, pmax_att=G, hbuf=4 * D, rgate=D, part_ffn=G, pmax_ffn=G, lnstat=6)[name]
        out = np.zeros(n, dt)
        _chk(lib().rwkv_debug_read(self._h, which, out.ctypes.data, out.nbytes))
        return out

    def debug_write(self, name, arr):
        which, dt = self.DBG[name]
        a = np.ascontiguousarray(arr, dt)
        _chk(lib().rwkv_debug_write(self._h, which, a.ctypes.data, a.nbytes))

    def close(self):
        if self._h:
            lib().rwkv_free(self._h)
            self._h = C.c_void_p()
            self.ready = False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
