"""Refused calls of the C ABI (include/rwkv_mi355x.h): every entry point answers a NULL pointer, a context in the wrong state and an
argument out of range with the documented status and a message that names the fault, BEFORE anything is launched -- the loaded
context's five state arrays and its logits buffer are bit-identical afterwards and a greedy decode from them gives the same ids.

One table: entry point, arguments, status, a piece of rwkv_last_error().  The contexts an argument names: "M" a loaded whole model
(L = 2, D = 64 -- the narrowest width with a chunk path -- max_ctx 8), "U" created but never loaded, "S" a stage context (layers
[0, 1) of the two: neither a whole model nor a head), "P" a whole model with a one-rank pipeline transport (max_ctx 32).  No case
feeds a bad value to a kernel: where an entry point has no check for a value, the table has no case for it."""
import ctypes as C

import pytest

from rwkv_cpp_accelerated_amd import modelfile as mf
from support import E_ARG, E_IO, E_STATE, GuardContexts, V, check_refused, eng  # noqa: F401

pytestmark = pytest.mark.gpu
L, D, MAXT = 2, 64, 8
u64 = C.c_uint64


def a(*v):
    return (u64 * len(v))(*v)


OK2, BAD2, NINE = a(1, 2), a(1, V), a(*[1] * (MAXT + 1))
OUT = (u64 * 64)()
LP, ENT, AM = (C.c_double * 4)(), (C.c_double * 4)(), (u64 * 4)()
MS, BY, LN = (C.c_double * 7)(), (u64 * 7)(), (C.c_uint32 * 7)()
BUF = (C.c_char * 4096)()
ID128 = (C.c_char * 128)()
NOPTRS = (C.c_void_p * mf.N_TENSORS)()
NEWCTX = C.pointer(C.c_void_p())
NOFILE = b"/nonexistent/model.bin"
NOT_LOADED, WHOLE, HEAD, NULL = "RWKV not loaded", "whole-model", "hold the head", "NULL"
TOKEN, TARGET = f"token id {V} out of range", f"target id {V} out of range"

CASES = [
    # ---- NULL context ----
    ("rwkv_create", (None, 0), E_ARG, NULL),
    ("rwkv_create", (NEWCTX, 9999), E_ARG, "out of range"),
    ("rwkv_set_layer_range", (None, 0, 1), E_ARG, NULL),
    ("rwkv_load_file", (None, NOFILE, 1), E_ARG, NULL),
    ("rwkv_load_tensors", (None, L, D, NOPTRS, 0, 1), E_ARG, NULL),
    ("rwkv_forward", (None, OK2, 2, 1), E_ARG, NULL),
    ("rwkv_stage_forward", (None, 1, 0, None), E_ARG, NULL),
    ("rwkv_set_state", (None, None, None, None, None, None, 1), E_ARG, NULL),
    ("rwkv_get_output", (None, None, None, None, None, None, None, 1), E_ARG, NULL),
    ("rwkv_reset_state", (None,), E_ARG, NULL),
    ("rwkv_decode_greedy", (None, 1, 4, OUT), E_ARG, NULL),
    ("rwkv_sample_typical", (None, 0, 0.9, 0.8, 0.5, 0, OUT), E_ARG, NULL),
    ("rwkv_decode_typical", (None, 1, 4, 0.9, 0.8, 3, 0, OUT), E_ARG, NULL),
    ("rwkv_decode_batch_greedy", (None, OK2, 2, 4, OUT), E_ARG, NULL),
    ("rwkv_decode_batch_typical", (None, OK2, 2, 4, 0.9, 0.8, OK2, 0, OUT), E_ARG, NULL),
    ("rwkv_state_copy", (None, 1, 0), E_ARG, NULL),
    ("rwkv_score_rows", (None, OK2, OK2, 2, LP, ENT, AM), E_ARG, NULL),
    ("rwkv_score", (None, OK2, OK2, 2, LP, ENT, AM), E_ARG, NULL),
    ("rwkv_profile_token", (None, 1, 1, MS, BY, LN), E_ARG, NULL),
    ("rwkv_profile_batched", (None, 1, 1, MS, LN), E_ARG, NULL),
    ("rwkv_debug_timeline", (None, 1, BUF, 512), E_ARG, NULL),
    ("rwkv_debug_launch", (None, 0, 0, 1, 0), E_ARG, NULL),
    ("rwkv_debug_read", (None, 0, BUF, 4096), E_ARG, NULL),
    ("rwkv_debug_write", (None, 0, BUF, D * 8), E_ARG, NULL),
    ("rwkv_stage_chunk", (None, OK2, 2, 0, 0), E_ARG, NULL),
    ("rwkv_sync", (None,), E_ARG, NULL),
    ("rwkv_xseq_copy", (None, 0, "M", 0, 1), E_ARG, "bad copy"),
    ("rwkv_pipe_init", (None, ID128, 0, 1), E_ARG, NULL),
    ("rwkv_pipe_info", (None, BUF, 4096), E_ARG, NULL),
    ("rwkv_pipe_decode_streams", (None, OK2, 1, 1, OUT), E_ARG, NULL),
    ("rwkv_pipe_decode_dual", (None, OK2, 1, OUT), E_ARG, NULL),
    ("rwkv_pipe_decode", (None, OK2, 1, OUT), E_STATE, "rwkv_pipe_init"),
    ("rwkv_pipe_profile", (None, 1), E_ARG, NULL),
    ("rwkv_pipe_hop_stats", (None, MS), E_ARG, NULL),
    ("rwkv_pipe_prefill", (None, OK2, 2), E_ARG, NULL),
    # ---- NULL array arguments ----
    ("rwkv_load_file", ("M", None, 1), E_ARG, NULL),
    ("rwkv_load_tensors", ("M", L, D, None, 0, 1), E_ARG, NULL),
    ("rwkv_forward", ("M", None, 2, 1), E_ARG, NULL),
    ("rwkv_decode_greedy", ("M", 1, 4, None), E_ARG, NULL),
    ("rwkv_sample_typical", ("M", 0, 0.9, 0.8, 0.5, 0, None), E_ARG, NULL),
    ("rwkv_decode_typical", ("M", 1, 4, 0.9, 0.8, 3, 0, None), E_ARG, NULL),
    ("rwkv_decode_batch_greedy", ("M", None, 2, 4, OUT), E_ARG, NULL),
    ("rwkv_decode_batch_greedy", ("M", OK2, 2, 4, None), E_ARG, NULL),
    ("rwkv_decode_batch_typical", ("M", None, 2, 4, 0.9, 0.8, OK2, 0, OUT), E_ARG, NULL),
    ("rwkv_decode_batch_typical", ("M", OK2, 2, 4, 0.9, 0.8, None, 0, OUT), E_ARG, NULL),
    ("rwkv_decode_batch_typical", ("M", OK2, 2, 4, 0.9, 0.8, OK2, 0, None), E_ARG, NULL),
    ("rwkv_score_rows", ("M", None, OK2, 2, LP, ENT, AM), E_ARG, NULL),
    ("rwkv_score_rows", ("M", OK2, None, 2, LP, ENT, AM), E_ARG, NULL),
    ("rwkv_score_rows", ("M", OK2, OK2, 2, None, ENT, AM), E_ARG, NULL),
    ("rwkv_score", ("M", None, OK2, 2, LP, ENT, AM), E_ARG, NULL),
    ("rwkv_score", ("M", OK2, None, 2, LP, ENT, AM), E_ARG, NULL),
    ("rwkv_score", ("M", OK2, OK2, 2, None, ENT, AM), E_ARG, NULL),
    ("rwkv_profile_token", ("M", 1, 1, None, BY, LN), E_ARG, NULL),
    ("rwkv_profile_batched", ("M", 1, 1, None, LN), E_ARG, NULL),
    ("rwkv_profile_batched", ("M", 1, 1, MS, None), E_ARG, NULL),
    ("rwkv_debug_timeline", ("M", 1, None, 1 << 20), E_ARG, NULL),
    ("rwkv_debug_read", ("M", 0, None, 4096), E_ARG, NULL),
    ("rwkv_debug_write", ("M", 0, None, D * 8), E_ARG, NULL),
    ("rwkv_stage_chunk", ("M", None, 2, 0, 0), E_ARG, "stage 0 needs the token ids"),
    ("rwkv_pipe_init", ("M", None, 0, 1), E_ARG, NULL),
    ("rwkv_pipe_info", ("P", None, 4096), E_ARG, NULL),
    ("rwkv_pipe_hop_stats", ("M", None), E_ARG, NULL),
    ("rwkv_pipe_decode_streams", ("P", None, 1, 1, OUT), E_ARG, "rank 0 needs first_tokens"),
    ("rwkv_pipe_decode_streams", ("P", OK2, 1, 1, None), E_ARG, "the last rank needs picks"),
    ("rwkv_pipe_decode_dual", ("P", None, 1, OUT), E_ARG, "rank 0 needs first_tokens"),
    ("rwkv_pipe_decode_dual", ("P", OK2, 1, None), E_ARG, "the last rank needs picks"),
    ("rwkv_pipe_prefill", ("P", None, 2), E_ARG, "empty prompt"),
    # ---- not loaded ----
    ("rwkv_forward", ("U", OK2, 2, 1), E_STATE, NOT_LOADED),
    ("rwkv_stage_forward", ("U", 1, 0, None), E_STATE, NOT_LOADED),
    ("rwkv_set_state", ("U", None, None, None, None, None, 1), E_STATE, NOT_LOADED),
    ("rwkv_get_output", ("U", None, None, None, None, None, None, 1), E_STATE, NOT_LOADED),
    ("rwkv_reset_state", ("U",), E_STATE, NOT_LOADED),
    ("rwkv_decode_greedy", ("U", 1, 4, OUT), E_STATE, NOT_LOADED),
    ("rwkv_sample_typical", ("U", 0, 0.9, 0.8, 0.5, 0, OUT), E_STATE, NOT_LOADED),
    ("rwkv_decode_typical", ("U", 1, 4, 0.9, 0.8, 3, 0, OUT), E_STATE, NOT_LOADED),
    ("rwkv_decode_batch_greedy", ("U", OK2, 2, 4, OUT), E_STATE, NOT_LOADED),
    ("rwkv_decode_batch_typical", ("U", OK2, 2, 4, 0.9, 0.8, OK2, 0, OUT), E_STATE, NOT_LOADED),
    ("rwkv_state_copy", ("U", 1, 0), E_STATE, NOT_LOADED),
    ("rwkv_score_rows", ("U", OK2, OK2, 2, LP, ENT, AM), E_STATE, NOT_LOADED),
    ("rwkv_score", ("U", OK2, OK2, 2, LP, ENT, AM), E_STATE, NOT_LOADED),
    ("rwkv_profile_token", ("U", 1, 1, MS, BY, LN), E_STATE, NOT_LOADED),
    ("rwkv_profile_batched", ("U", 1, 1, MS, LN), E_STATE, NOT_LOADED),
    ("rwkv_debug_timeline", ("U", 1, BUF, 512), E_STATE, NOT_LOADED),
    ("rwkv_debug_launch", ("U", 0, 0, 1, 0), E_STATE, NOT_LOADED),
    ("rwkv_debug_read", ("U", 0, BUF, 4096), E_STATE, NOT_LOADED),
    ("rwkv_debug_write", ("U", 0, BUF, D * 8), E_STATE, NOT_LOADED),
    ("rwkv_stage_chunk", ("U", OK2, 2, 0, 0), E_STATE, NOT_LOADED),
    ("rwkv_pipe_init", ("U", ID128, 0, 1), E_STATE, NOT_LOADED),
    ("rwkv_pipe_decode_streams", ("U", OK2, 1, 1, OUT), E_STATE, "loaded"),
    ("rwkv_pipe_decode_dual", ("U", OK2, 1, OUT), E_STATE, "loaded"),
    ("rwkv_pipe_prefill", ("U", OK2, 2), E_STATE, "loaded"),
    ("rwkv_xseq_copy", ("M", 0, "U", 0, 1), E_ARG, "bad copy"),
    # ---- loaded, but no pipeline transport; a transport that is there already ----
    ("rwkv_pipe_info", ("M", BUF, 4096), E_STATE, "rwkv_pipe_init"),
    ("rwkv_pipe_decode", ("M", OK2, 1, OUT), E_STATE, "rwkv_pipe_init"),
    ("rwkv_pipe_decode_streams", ("M", OK2, 1, 1, OUT), E_STATE, "rwkv_pipe_init"),
    ("rwkv_pipe_decode_dual", ("M", OK2, 1, OUT), E_STATE, "rwkv_pipe_init"),
    ("rwkv_pipe_prefill", ("M", OK2, 2), E_STATE, "rwkv_pipe_init"),
    ("rwkv_pipe_init", ("P", ID128, 0, 1), E_STATE, "already initialised"),
    # ---- loaded already ----
    ("rwkv_set_layer_range", ("M", 0, 1), E_STATE, "already loaded"),
    ("rwkv_load_tensors", ("M", L, D, NOPTRS, 0, 1), E_STATE, "already loaded"),
    ("rwkv_load_file", ("M", NOFILE, 1), E_IO, "Error opening file /nonexistent/model.bin"),
    ("rwkv_load_file", ("U", NOFILE, 1), E_IO, "Error opening file /nonexistent/model.bin"),
    ("rwkv_set_layer_range", ("U", 1, 1), E_ARG, "empty layer range"),
    # ---- a stage context where a whole model or a head is required ----
    ("rwkv_decode_greedy", ("S", 1, 4, OUT), E_STATE, WHOLE),
    ("rwkv_decode_typical", ("S", 1, 4, 0.9, 0.8, 3, 0, OUT), E_STATE, WHOLE),
    ("rwkv_decode_batch_greedy", ("S", OK2, 2, 4, OUT), E_STATE, WHOLE),
    ("rwkv_decode_batch_greedy", ("S", OK2, 1, 4, OUT), E_STATE, WHOLE),
    ("rwkv_decode_batch_typical", ("S", OK2, 2, 4, 0.9, 0.8, OK2, 0, OUT), E_STATE, WHOLE),
    ("rwkv_score", ("S", OK2, OK2, 2, LP, ENT, AM), E_STATE, WHOLE),
    ("rwkv_sample_typical", ("S", 0, 0.9, 0.8, 0.5, 0, OUT), E_STATE, HEAD),
    ("rwkv_score_rows", ("S", OK2, OK2, 2, LP, ENT, AM), E_STATE, HEAD),
    ("rwkv_debug_launch", ("S", 5, 0, 1, 0), E_STATE, HEAD),
    ("rwkv_debug_launch", ("S", 6, 0, 1, 0), E_STATE, HEAD),
    ("rwkv_debug_launch", ("S", 1, 1, 1, 0), E_ARG, "layer 1 is not one of this context's"),
    ("rwkv_pipe_init", ("S", ID128, 0, 1), E_ARG, "does not match this context's layer range"),
    # ---- a token or target id of 50277 ----
    ("rwkv_forward", ("M", BAD2, 2, 1), E_ARG, TOKEN),
    ("rwkv_forward", ("M", BAD2, 2, 0), E_ARG, TOKEN),
    ("rwkv_stage_forward", ("M", V, 0, None), E_ARG, TOKEN),
    ("rwkv_decode_greedy", ("M", V, 4, OUT), E_ARG, TOKEN),
    ("rwkv_decode_typical", ("M", V, 4, 0.9, 0.8, 3, 0, OUT), E_ARG, TOKEN),
    ("rwkv_decode_batch_greedy", ("M", BAD2, 2, 4, OUT), E_ARG, TOKEN),
    ("rwkv_decode_batch_greedy", ("M", a(V), 1, 4, OUT), E_ARG, TOKEN),
    ("rwkv_decode_batch_typical", ("M", BAD2, 2, 4, 0.9, 0.8, OK2, 0, OUT), E_ARG, TOKEN),
    ("rwkv_score_rows", ("M", OK2, BAD2, 2, LP, ENT, AM), E_ARG, TARGET),
    ("rwkv_score", ("M", BAD2, OK2, 2, LP, ENT, AM), E_ARG, TOKEN),
    ("rwkv_score", ("M", OK2, BAD2, 2, LP, ENT, AM), E_ARG, TARGET),
    ("rwkv_profile_token", ("M", V, 1, MS, BY, LN), E_ARG, "bad token"),
    ("rwkv_profile_batched", ("M", V, 1, MS, LN), E_ARG, "bad token"),
    ("rwkv_debug_launch", ("M", 0, 0, V, 0), E_ARG, TOKEN),
    ("rwkv_stage_chunk", ("M", BAD2, 2, 0, 0), E_ARG, TOKEN),
    ("rwkv_stage_chunk", ("S", BAD2, 2, 0, 0), E_ARG, TOKEN),
    # ---- zero counts and counts over the cap ----
    ("rwkv_forward", ("M", NINE, MAXT + 1, 1), E_ARG, "Context too large, max context is 8"),
    ("rwkv_forward", ("M", NINE, MAXT + 1, 0), E_ARG, "Context too large, max context is 8"),
    ("rwkv_set_state", ("M", None, None, None, None, None, MAXT + 1), E_ARG, "max context 8"),
    ("rwkv_get_output", ("M", None, None, None, None, None, None, MAXT + 1), E_ARG, "max context 8"),
    ("rwkv_decode_greedy", ("M", 1, 0, OUT), E_ARG, "n_tokens must be in 1..65536"),
    ("rwkv_decode_greedy", ("M", 1, 65537, OUT), E_ARG, "n_tokens must be in 1..65536"),
    ("rwkv_decode_typical", ("M", 1, 0, 0.9, 0.8, 3, 0, OUT), E_ARG, "n_tokens must be in 1..65536"),
    ("rwkv_decode_typical", ("M", 1, 65537, 0.9, 0.8, 3, 0, OUT), E_ARG, "n_tokens must be in 1..65536"),
    ("rwkv_decode_batch_greedy", ("M", OK2, 0, 4, OUT), E_ARG, "n_streams must be in 1..8"),
    ("rwkv_decode_batch_greedy", ("M", NINE, MAXT + 1, 4, OUT), E_ARG, "n_streams must be in 1..8"),
    ("rwkv_decode_batch_greedy", ("M", OK2, 2, 0, OUT), E_ARG, "n_steps must be in 1..65536"),
    ("rwkv_decode_batch_greedy", ("M", OK2, 2, 65537, OUT), E_ARG, "n_steps must be in 1..65536"),
    ("rwkv_decode_batch_greedy", ("M", OK2, 1, 65537, OUT), E_ARG, "n_steps must be in 1..65536"),
    ("rwkv_decode_batch_typical", ("M", OK2, 0, 4, 0.9, 0.8, OK2, 0, OUT), E_ARG, "n_streams must be in 1..8"),
    ("rwkv_decode_batch_typical", ("M", NINE, MAXT + 1, 4, 0.9, 0.8, NINE, 0, OUT), E_ARG, "n_streams must be in 1..8"),
    ("rwkv_decode_batch_typical", ("M", OK2, 2, 0, 0.9, 0.8, OK2, 0, OUT), E_ARG, "n_steps must be in 1..65536"),
    ("rwkv_decode_batch_typical", ("M", OK2, 2, 65537, 0.9, 0.8, OK2, 0, OUT), E_ARG, "n_steps must be in 1..65536"),
    ("rwkv_score_rows", ("M", OK2, OK2, 0, LP, ENT, AM), E_ARG, "must be in 1..65536"),
    ("rwkv_score_rows", ("M", OK2, OK2, 65537, LP, ENT, AM), E_ARG, "must be in 1..65536"),
    ("rwkv_score", ("M", OK2, OK2, 0, LP, ENT, AM), E_ARG, "must be in 1..65536"),
    ("rwkv_score", ("M", OK2, OK2, 65537, LP, ENT, AM), E_ARG, "must be in 1..65536"),
    ("rwkv_profile_token", ("M", 1, 0, MS, BY, LN), E_ARG, "reps"),
    ("rwkv_profile_batched", ("M", 1, 0, MS, LN), E_ARG, "reps"),
    ("rwkv_debug_timeline", ("M", 1, BUF, 512), E_ARG, "need room for"),
    ("rwkv_stage_chunk", ("M", OK2, 0, 0, 0), E_ARG, "bad chunk"),
    ("rwkv_stage_chunk", ("M", NINE, 65, 0, 0), E_ARG, "bad chunk"),
    ("rwkv_stage_chunk", ("M", NINE, MAXT + 1, 0, 0), E_ARG, "bad chunk"),
    ("rwkv_stage_chunk", ("M", OK2, 2, MAXT - 1, 0), E_ARG, "bad chunk"),
    ("rwkv_stage_chunk", ("M", OK2, 2, 0, 2), E_ARG, "bad chunk"),
    ("rwkv_xseq_copy", ("M", 0, "S", 0, 65), E_ARG, "bad copy"),
    ("rwkv_pipe_init", ("M", ID128, 1, 1), E_ARG, "bad rank 1 of 1"),
    ("rwkv_pipe_init", ("M", ID128, 0, 0), E_ARG, "bad rank 0 of 0"),
    ("rwkv_pipe_init", ("M", ID128, 0, 2), E_ARG, "does not match this context's layer range"),
    ("rwkv_pipe_decode_streams", ("P", OK2, 1, 0, OUT), E_ARG, "n_streams must be in 1..world"),
    ("rwkv_pipe_decode_streams", ("P", OK2, 1, 2, OUT), E_ARG, "n_streams must be in 1..world"),
    ("rwkv_pipe_decode_streams", ("P", OK2, 0, 1, OUT), E_ARG, "world * n_steps must be in 1..65536"),
    ("rwkv_pipe_decode_streams", ("P", OK2, 65537, 1, OUT), E_ARG, "world * n_steps must be in 1..65536"),
    ("rwkv_pipe_decode", ("P", OK2, 0, OUT), E_ARG, "world * n_steps must be in 1..65536"),
    ("rwkv_pipe_decode_dual", ("P", OK2, 0, OUT), E_ARG, "2 * world * n_steps must be in 1..65536"),
    ("rwkv_pipe_decode_dual", ("P", OK2, 32769, OUT), E_ARG, "2 * world * n_steps must be in 1..65536"),
    ("rwkv_pipe_prefill", ("P", OK2, 0), E_ARG, "empty prompt"),
    # ---- slot and row equal to max_ctx ----
    ("rwkv_stage_forward", ("M", 1, MAXT, None), E_ARG, "state slot 8 out of range"),
    ("rwkv_sample_typical", ("M", MAXT, 0.9, 0.8, 0.5, 0, OUT), E_ARG, "logits row 8 out of range"),
    ("rwkv_state_copy", ("M", MAXT, 0), E_ARG, "state slot out of range"),
    ("rwkv_state_copy", ("M", 0, MAXT), E_ARG, "state slot out of range"),
    ("rwkv_score_rows", ("M", a(0, MAXT), OK2, 2, LP, ENT, AM), E_ARG, "logits row 8 out of range"),
    ("rwkv_debug_launch", ("M", 0, 0, 1, MAXT), E_ARG, "state slot 8 out of range"),
    # ---- temp = 0, u = 1, a bad mode ----
    ("rwkv_sample_typical", ("M", 0, 0.0, 0.8, 0.5, 0, OUT), E_ARG, "temp > 0"),
    ("rwkv_sample_typical", ("M", 0, 0.9, 0.8, 1.0, 0, OUT), E_ARG, "u < 1"),
    ("rwkv_sample_typical", ("M", 0, 0.9, 0.8, -0.5, 0, OUT), E_ARG, "0 <= u"),
    ("rwkv_decode_typical", ("M", 1, 4, 0.0, 0.8, 3, 0, OUT), E_ARG, "temp > 0"),
    ("rwkv_decode_typical", ("M", 1, 4, float("nan"), 0.8, 3, 0, OUT), E_ARG, "temp > 0"),
    ("rwkv_decode_batch_typical", ("M", OK2, 2, 4, 0.0, 0.8, OK2, 0, OUT), E_ARG, "temp > 0"),
    ("rwkv_decode_batch_typical", ("M", OK2, 1, 4, 0.0, 0.8, OK2, 0, OUT), E_ARG, "temp > 0"),
    ("rwkv_forward", ("M", OK2, 2, 2), E_ARG, "bad mode 2"),
    ("rwkv_forward", ("M", OK2, 2, -1), E_ARG, "bad mode -1"),
    # ---- a debug buffer or kernel class out of range, a debug buffer with the wrong size ----
    ("rwkv_debug_read", ("M", 9, BUF, 4096), E_ARG, "no such debug buffer: 9"),
    ("rwkv_debug_read", ("M", -1, BUF, 4096), E_ARG, "no such debug buffer: -1"),
    ("rwkv_debug_write", ("M", 9, BUF, D * 8), E_ARG, "no such debug buffer: 9"),
    ("rwkv_debug_read", ("M", 0, BUF, D * 8 - 1), E_ARG, "debug buffer 0 holds 512 bytes"),
    ("rwkv_debug_write", ("M", 0, BUF, D * 8 - 8), E_ARG, "debug buffer 0 holds 512 bytes"),
    ("rwkv_debug_write", ("M", 8, BUF, 6 * 8 + 8), E_ARG, "debug buffer 8 holds 48 bytes"),
    ("rwkv_debug_launch", ("M", 7, 0, 1, 0), E_ARG, "kernel class 7 out of range"),
    ("rwkv_debug_launch", ("M", -1, 0, 1, 0), E_ARG, "kernel class -1 out of range"),
    ("rwkv_debug_launch", ("M", 1, L, 1, 0), E_ARG, "layer 2 is not one of this context's"),
    # ---- two faults at once: the first check in the entry point's order answers ----
    ("rwkv_decode_greedy", ("U", 1, 4, None), E_ARG, NULL),                         # NULL array before "not loaded"
    ("rwkv_score", ("U", OK2, OK2, 2, None, ENT, AM), E_ARG, NULL),
    ("rwkv_decode_batch_typical", ("S", OK2, 2, 4, 0.9, 0.8, None, 0, OUT), E_ARG, NULL),
    ("rwkv_decode_greedy", ("U", V, 0, OUT), E_STATE, NOT_LOADED),                  # "not loaded" before the call's own arguments
    ("rwkv_forward", ("U", NINE, MAXT + 1, 2), E_STATE, NOT_LOADED),
    ("rwkv_decode_greedy", ("S", V, 0, OUT), E_STATE, WHOLE),                       # whole model / head before the call's own arguments
    ("rwkv_sample_typical", ("S", MAXT, 0.0, 0.8, 1.0, 0, OUT), E_STATE, HEAD),
    ("rwkv_score_rows", ("S", OK2, BAD2, 0, LP, ENT, AM), E_STATE, HEAD),
    ("rwkv_forward", ("M", NINE, MAXT + 1, 2), E_ARG, "Context too large"),         # the call's own arguments in the order of the entry point
    ("rwkv_forward", ("M", BAD2, 2, 2), E_ARG, "bad mode 2"),
    ("rwkv_decode_greedy", ("M", V, 0, OUT), E_ARG, TOKEN),
    ("rwkv_decode_typical", ("M", 1, 0, 0.0, 0.8, 3, 0, OUT), E_ARG, "n_tokens must be in"),
    ("rwkv_decode_batch_greedy", ("M", BAD2, 2, 0, OUT), E_ARG, "n_steps must be in"),
    ("rwkv_decode_batch_typical", ("M", BAD2, 2, 4, 0.0, 0.8, OK2, 0, OUT), E_ARG, TOKEN),
    ("rwkv_stage_forward", ("M", V, MAXT, None), E_ARG, "state slot 8 out of range"),
    ("rwkv_debug_launch", ("M", 7, L, V, MAXT), E_ARG, "kernel class 7 out of range"),
    ("rwkv_debug_read", ("M", 9, None, 0), E_ARG, NULL),
    ("rwkv_pipe_decode_streams", ("P", None, 0, 0, None), E_ARG, "n_streams must be in 1..world"),
]


def _case_id(i):
    entry, args = CASES[i][0], CASES[i][1]
    return f"{i:03d}-{entry[5:]}-{args[0] if isinstance(args[0], str) else 'null'}"


@pytest.fixture(scope="module")
def ctx(eng):
    x = GuardContexts(eng, L, D, MAXT, extra=("P",))
    yield x
    x.close()


@pytest.mark.parametrize("i", range(len(CASES)), ids=_case_id)
def test_a_refused_call_answers_its_status_and_launches_nothing(ctx, i):
    entry, args, status, text = CASES[i]
    check_refused(ctx, entry, [ctx.h[v] if isinstance(v, str) else v for v in args], status, text)
