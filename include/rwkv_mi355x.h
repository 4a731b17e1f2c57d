/*
 * rwkv_mi355x.h -- C-ABI of the MI355X-native RWKV-v4 uint8 inference engine
 * (librwkv_mi355x.so).  Plain pointers and sizes only; no C++ or torch types.
 *
 * This is the drop-in boundary that sits where the reference's backend link
 * boundary sits: the seven C++-linkage free functions that reference
 * include/rwkv/rwkv/rwkv.h:63-122 declares and include/rwkv/cuda/rwkv.cu
 * defines.  The 46-pointer interface of the reference is replaced by an opaque
 * handle; each entry point cites the reference function it replaces.
 * The C++ drop-in header include/rwkv.h (class RWKV / RWKVState) and the pybind
 * module `rwkv` are thin wrappers over these calls.
 *
 * All functions return 0 on success and a negative rwkv_status on failure;
 * rwkv_last_error() gives a human-readable message for the calling thread.
 * Nothing here falls back to a CPU path: without a gfx950 device every
 * compute entry point fails with RWKV_E_DEVICE.
 */
#ifndef RWKV_MI355X_H
#define RWKV_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this C-ABI: bumped whenever an existing entry point changes its argument list or meaning (additions alone do
 * not bump it).  3: rwkv_decode_typical / rwkv_sample_typical take `flags`; the one-launch-token hooks (rwkv_one_launch,
 * rwkv_debug_mega_timeline) are gone; bounded device-side waits report RWKV_E_DEVICE.  4: weight rows carried in LDS that fail
 * their check are re-loaded instead of failing the call (no more "arrived damaged" error); the carry counters are on by default
 * (rwkv_debug_carry_stats).  5: the two-communicator pipeline schedule.  6: the weight rows carried in LDS across kernel boundaries
 * are gone and with them rwkv_debug_carry_stats / rwkv_debug_carry_hits; the stand-alone GEMV entry point rwkv_mm8_one -- a kernel that only the tests launched -- is
 * replaced by rwkv_debug_launch / rwkv_debug_read / rwkv_debug_write, which run and inspect the PRODUCTION decode kernels one at a time.
 * rwkv_abi_version() returns the value the
 * library was built with: a binding compares it with the header it was compiled against. */
#define RWKV_MI355X_ABI_VERSION 6
int rwkv_abi_version(void);

#define RWKV_VOCAB 50277u /* hard-wired in the reference: rwkv.h:126, rwkv.cu:471,589 */
#define RWKV_N_TENSORS 46 /* tensor slots of model.bin: enums/enum.h:7-55 */

enum rwkv_mode { RWKV_MODE_PARRALEL = 0, RWKV_MODE_GPT = 1 }; /* enums/enum.h:2-5 (sic) */

enum rwkv_status {
    RWKV_OK = 0,
    RWKV_E_ARG = -1,    /* bad argument (reference: std::runtime_error in rwkv.h:285,344,349) */
    RWKV_E_IO = -2,     /* file missing / truncated (reference: exit(1), rwkv.cu:641-645) */
    RWKV_E_DEVICE = -3, /* HIP error or no usable device (reference: unchecked) */
    RWKV_E_STATE = -4   /* called in the wrong state (not loaded / already loaded) */
};

typedef struct rwkv_ctx rwkv_ctx;

/* State arrays addressable through rwkv_state_device(). */
enum rwkv_state_id { RWKV_STATE_XY = 0, RWKV_STATE_AA = 1, RWKV_STATE_BB = 2, RWKV_STATE_PP = 3, RWKV_STATE_DD = 4 };

/* Create an empty context bound to HIP device `device`.  (No reference counterpart:
 * the reference uses the process-default device.) */
int rwkv_create(rwkv_ctx **out, int device);

/* Replaces load(), rwkv.cu:638-717: read model.bin (2 x u64 header,
 * 46 raw tensors), upload, re-tile the uint8 matrices into the engine's row-per-output
 * layout, allocate scratch and state for `max_ctx` tokens/slots (the reference's maxGPT). */
int rwkv_load_file(rwkv_ctx *ctx, const char *path, uint64_t max_ctx);

/* Same as rwkv_load_file but from memory: `ptrs[i]` is tensor slot i in FILE layout
 * (host memory if on_device == 0, device memory otherwise).  The 13 scratch/state slots
 * may be NULL.  Used by the converter path and by bench.py's synthetic 7B/14B models. */
int rwkv_load_tensors(rwkv_ctx *ctx, uint64_t n_layers, uint64_t n_embed,
                      const void *const *ptrs, int on_device, uint64_t max_ctx);

uint64_t rwkv_n_layers(const rwkv_ctx *ctx);
uint64_t rwkv_n_embed(const rwkv_ctx *ctx);
uint64_t rwkv_max_ctx(const rwkv_ctx *ctx);

/* Replaces cuda_rwkv_parralel(), rwkv.cu:493-593 (and cuda_rwkv, :595-628): run `n_tokens`
 * tokens.  GPT mode: consecutive tokens of one sequence on state slot 0.  PARRALEL mode: one
 * step of n_tokens independent sequences on state slots 0..n_tokens-1.  Logits for every
 * position land in the device logits buffer ([n_tokens][50277] f32); state stays on the device.
 * n_tokens == 1 runs the decode kernels (uint8 x fixed-point dot products on the VALU); n_tokens >= 2
 * on a whole-model context with max_ctx > 1 runs mm8_seq on the int8 matrix cores in weight passes of up
 * to 64 rows (two 32-row halves that share every weight fragment; a call of <= 32 rows, or env
 * RWKV_SEQ_ROWS=32: one 32-row chunk per pass), every weight byte read once per pass, the passes of a
 * longer call pipelined over RWKV_SEQ_STAGES (default 3) streams of the one GPU (env RWKV_SEQ=0 at load
 * time keeps the token-by-token path).  All schedules give bit-identical results and agree with the
 * reference within its own tolerance; see DESIGN.md 5.
 * Synchronous on return (the reference ends with cudaDeviceSynchronize, rwkv.cu:590). */
int rwkv_forward(rwkv_ctx *ctx, const uint64_t *tokens, uint64_t n_tokens, int mode);

/* Replaces setState(), rwkv.cu:479-490: upload host state arrays (each [n_slots][L][D] f64). */
int rwkv_set_state(rwkv_ctx *ctx, const double *xy, const double *aa, const double *bb,
                   const double *pp, const double *dd, uint64_t n_slots);

/* Replaces getOutput(), rwkv.cu:467-477: download logits ([n_tokens][50277] f32) and the five
 * state arrays (each [n_tokens][L][D] f64).  Any pointer may be NULL to skip that copy. */
int rwkv_get_output(rwkv_ctx *ctx, float *logits, double *xy, double *aa, double *bb,
                    double *pp, double *dd, uint64_t n_tokens);

/* Zero all state slots on the device (what `new RWKVState` + setState does, rwkv.h:163-170). */
int rwkv_reset_state(rwkv_ctx *ctx);

/* Device-side greedy continuation (storygen's loop, examples/storygen/storygen.cpp:63-69, with
 * argmax in place of typical(): logit 0 is banned as out[0] = -99 does there).  Feeds
 * `first_token`, then n_tokens-1 times the argmax of the previous logits, all on state slot 0
 * without host round trips; writes the n_tokens picked ids to out_tokens (host).  The logits of
 * the LAST step remain in the device logits buffer (row 0). */
int rwkv_decode_greedy(rwkv_ctx *ctx, uint64_t first_token, uint64_t n_tokens, uint64_t *out_tokens);

/* The reference's sampler typical() (include/rwkv/sampler/typical.h:20-58) on the device, from the logits row
 * `row` of the LAST forward, without downloading them.  The draw is the inverse CDF in token order for the
 * caller's uniform u in [0, 1) (include/rwkv_sampler.h typical_u() is the same draw on the host).
 * Default = what typical.h COMPUTES (pinned by tests/test_sampler_ref_cpu.py against 20 000 draws of the
 * reference's own function per case): a draw from softmax(logits)^n with n = uint8(1/temp) -- its typical-set cut
 * at tau assigns into a temporary and has no effect (typical.h:50) and nc::power takes an integer exponent
 * (typical.h:52); n = 0 (temp > 1) is the uniform distribution.  RWKV_SAMPLE_RECIPE instead applies the recipe its
 * header comment documents (entropy, |-log p - H| ordering, smallest prefix with cumulative probability >= tau,
 * p^(1/temp)).  RWKV_SAMPLE_BAN0 first sets logit 0 to -99 as storygen does (examples/storygen/storygen.cpp:66).
 * GUARANTEED for every temp > 0: the weights are formed relative to the largest one of the kept set, which is therefore never
 * lost to underflow -- near-greedy temperatures (temp 0.01, n = 100) draw from the kept set like any other, where p^n itself is
 * below f32 and f64 for every token (the host typical_u() returns 0 there: include/rwkv_sampler.h).  The pick is a kept token;
 * id 0 comes back only where the reference's arithmetic picks it (with BAN0: when -99 still is the largest logit, or in default
 * mode at temp > 1, where n = 0 weighs every id alike).  Held draw by draw to a log-space f64 evaluation on planted logits by
 * tests/test_sampler_cases_gpu.py. */
#define RWKV_SAMPLE_BAN0 1
#define RWKV_SAMPLE_RECIPE 2
int rwkv_sample_typical(rwkv_ctx *ctx, uint64_t row, float temp, float tau, double u, int flags, uint64_t *token);

/* Device-side sampled continuation: storygen's loop (examples/storygen/storygen.cpp:63-69: forward, out[0] = -99,
 * typical) with the sampler above in place of the host typical(); u of step k = uniform(splitmix64(seed + k));
 * flags: RWKV_SAMPLE_RECIPE (logit 0 is always banned here).  Same contract as rwkv_decode_greedy otherwise. */
int rwkv_decode_typical(rwkv_ctx *ctx, uint64_t first_token, uint64_t n_tokens, float temp, float tau,
                        uint64_t seed, int flags, uint64_t *out_tokens);

/* ---- batched decode: N independent streams, one weight pass per step (no reference counterpart: SURVEY.md 2) ----
 * Device-side continuation of n_streams independent sequences: stream s runs on state slot s (PARRALEL mode's mapping,
 * rwkv.cu:236-240), is fed first_tokens[s], then n_steps - 1 times its own previous pick -- per stream exactly the contract of
 * rwkv_decode_greedy (logit 0 banned, ties -> lowest id, no winner -> 0).  out_tokens is host [n_streams][n_steps].  The logits of
 * the LAST step remain in the device logits buffer, rows 0 .. n_streams - 1.
 * n_streams == 1 runs rwkv_decode_greedy itself (the decode kernels on slot 0).  For n_streams >= 2 every step is the schedule of
 * rwkv_forward(n_streams tokens, RWKV_MODE_PARRALEL) -- passes of <= 64 rows, the RWKV_SEQ_STAGES pipeline for more than one pass,
 * the same kernels, so bit-identical logits -- except that the embedding reads the step's ids from the device, where the previous
 * step's pick over all rows left them.  Inside the loop there is no host synchronisation and no host <-> device copy: one upload of
 * first_tokens (and seeds), one download of all picks.  The picks and the per-row pick scratch belong to the context: allocated at
 * the first call, grown to the largest n_streams x n_steps seen, counted by rwkv_resident_bytes, freed by rwkv_free.
 * Status: RWKV_E_ARG for a NULL pointer, n_streams == 0 or > max_ctx, n_steps == 0 or > RWKV_MAX_DECODE_STEPS, a token id >= 50277
 * or !(temp > 0); RWKV_E_STATE when not loaded, on a pipeline-stage context, or for n_streams >= 2 without the chunk path (env
 * RWKV_SEQ=0 at load time, max_ctx 1, or an n_embed that is not a multiple of 64: the chunk path exists for the 80 widths 64, 128,
 * ... 5120, and the other multiples of 16 that load run every call token by token).  Every check runs before anything is launched: a rejected call leaves the state as it was. */
#define RWKV_MAX_DECODE_STEPS 65536u
int rwkv_decode_batch_greedy(rwkv_ctx *ctx, const uint64_t *first_tokens, uint64_t n_streams, uint64_t n_steps,
                             uint64_t *out_tokens);
/* Same with the device sampler: stream s draws u_k = uniform(splitmix64(seeds[s] + k)) at step k, i.e. the draws that
 * rwkv_decode_typical(seed = seeds[s]) makes; flags: RWKV_SAMPLE_RECIPE (logit 0 is always banned, as there).  One launch of each
 * of the sampler's three kernels covers all n_streams rows per step. */
int rwkv_decode_batch_typical(rwkv_ctx *ctx, const uint64_t *first_tokens, uint64_t n_streams, uint64_t n_steps,
                              float temp, float tau, const uint64_t *seeds, int flags, uint64_t *out_tokens);
/* Device-to-device copy of the five state arrays of slot src_slot into slot dst_slot: fork a prompt prefilled on slot 0 into the
 * slots of a batched decode.  RWKV_E_ARG for a slot >= max_ctx, RWKV_E_STATE when not loaded. */
int rwkv_state_copy(rwkv_ctx *ctx, uint64_t dst_slot, uint64_t src_slot);

/* ---- nucleus sampling with repetition penalties, on the device (no reference counterpart: the reference ships typical() only) ----
 * What the front ends of RWKV-4 models sample with: temperature, top-p, optionally top-k, presence and frequency penalties on a decaying
 * occurrence count.  For one logits row l (f32, widened to f64) and one count vector c (f32 [50277], the occurrence counts of one stream):
 *   1. penalty  l'_i = l_i - (presence + c_i * frequency) where c_i > 0, l'_i = l_i otherwise; with RWKV_NUCLEUS_BAN0 then l'_0 = -99 (storygen's
 *               out[0] = -99, applied after the penalty).  With presence == 0 and frequency == 0 counts are not read, updated or allocated
 *   2. softmax  p = softmax(l'), f64
 *   3. top-p    order by descending p (stable in token id); v = p at the first position where the running mass reaches top_p; every token with
 *               p_i >= v is kept (ties at the cut too).  top_p <= 0 keeps the most probable token and its ties; a mass that never reaches top_p
 *               (top_p >= 1) keeps everything
 *   4. top-k    with 0 < top_k < 50277 only tokens with p_i >= the top_k-th largest p are kept (ties too); 0 or >= 50277: off; 1 is penalised
 *               greedy (among exact ties u decides)
 *   5. kept     the intersection of 3 and 4; the most probable token is always in it
 *   6. weights  exp((l'_i - max l') / temp) on the kept set: the largest weight is exactly 1 at every temp > 0, nothing underflows
 *   7. draw     inverse CDF in token order for u in [0, 1); in the loops u of step k = uniform(splitmix64(seed + k)), the generator of the typical loops
 *   8. counts   after the pick g, when updating: c_i <- f32(c_i * decay) for every i, then c_g <- c_g + 1, in f32 (a host restatement is bit-exact)
 * On the device the cuts compare -log p as f32 (csrc/nucleus.hip.h): tokens whose p agree to 2^-23 relative tie.  Held draw by draw to a log-space
 * f64 evaluation on planted logits by tests/test_nucleus_gpu.py; include/rwkv_sampler.h nucleus_u is the same draw on the host.  With NaN or +inf
 * logits the pick is unspecified but below 50277, and nothing faults.
 *
 * The counts are one [max_ctx][50277] f32 buffer of the context, one vector per state slot: allocated and zeroed at the first call that needs it,
 * counted by rwkv_resident_bytes, freed with the context; they persist across steps and calls.  The two copy calls below move one vector (201 KB)
 * from / to host memory -- save and restore a chat session, count a prompt's tokens on the host and upload them; counts == NULL in the set call zeroes the vector.
 *
 * The sample call draws from logits row `row` of the LAST forward with the counts of state slot `slot` (independent of each other), updates
 * the counts only with RWKV_NUCLEUS_UPDATE, and leaves logits and state alone.  The two decode calls follow the contracts of the typical loops above
 * (stream s on slot s, logit 0 always banned, one upload and one download, no host synchronisation inside, n_streams == 1 on the decode kernels,
 * more on the chunk path); they always update the counts, and zero those of their slots first unless RWKV_NUCLEUS_KEEP is set: with it a 16-step
 * call gives exactly the ids of an 8-step call followed by an 8-step KEEP call with seed + 8.
 * Status: RWKV_E_ARG for a NULL pointer, !(temp > 0), a non-finite top_p, presence or frequency, decay outside [0, 1], unknown flag bits or
 * reserved != 0, u outside [0, 1), a row or slot >= max_ctx, a token id >= 50277, a step or stream count out of range; RWKV_E_STATE as for the
 * typical calls.  Every check runs before anything is launched or allocated: a rejected call leaves state, logits and counts as they were. */
#define RWKV_NUCLEUS_BAN0 1u
#define RWKV_NUCLEUS_KEEP 2u
#define RWKV_NUCLEUS_UPDATE 4u
typedef struct rwkv_nucleus_params {
    float temp, top_p;
    uint32_t top_k;
    float presence, frequency, decay;
    uint32_t flags;    /* RWKV_NUCLEUS_BAN0 | RWKV_NUCLEUS_KEEP | RWKV_NUCLEUS_UPDATE */
    uint32_t reserved; /* must be 0 */
} rwkv_nucleus_params;
int rwkv_sample_nucleus(rwkv_ctx *ctx, uint64_t row, uint64_t slot, const rwkv_nucleus_params *params, double u, uint64_t *token);
int rwkv_decode_nucleus(rwkv_ctx *ctx, uint64_t first_token, uint64_t n_tokens, const rwkv_nucleus_params *params, uint64_t seed,
                        uint64_t *out_tokens);
int rwkv_decode_batch_nucleus(rwkv_ctx *ctx, const uint64_t *first_tokens, uint64_t n_streams, uint64_t n_steps,
                              const rwkv_nucleus_params *params, const uint64_t *seeds, uint64_t *out_tokens);
int rwkv_penalty_set(rwkv_ctx *ctx, uint64_t slot, const float *counts /* host [50277]; NULL: zero */);
int rwkv_penalty_get(rwkv_ctx *ctx, uint64_t slot, float *counts /* host [50277] */);

/* ---- stop sequences and per-stream budgets in the device decode loops (no reference counterpart: its chat loops stop on the host) ----
 * The three batch calls above run every stream for exactly n_steps tokens.  This one ends each stream where a serving caller wants it
 * ended -- at a stop sequence ("\n\n", "Bob:", "User:": one to a few tokens) or at the stream's own token budget -- still without a host
 * round trip per token, and leaves every stream in exactly the condition it had when it stopped.
 *
 * Picks.  Stream s runs on slot s and produces the picks g_0, g_1, ... of the matching rwkv_decode_batch_greedy / _typical / _nucleus
 * call: the same kernels, the same seeds and u of step k, logit 0 always banned; n_streams == 1 runs the decode kernels, as there.
 * Stopping.  After pick g_k stream s stops when some stop sequence j equals the newest seq_len[j] ids of its history ..., first_token,
 * g_0 ... g_k, or when k + 1 == max_new[s].  A match ends at a generated token; it may begin in first_token or, with RWKV_STOP_KEEP, in
 * earlier calls.  out_len[s] = k + 1.  out_reason[s]: 0 the stream ran all n_steps (a budget equal to n_steps is this case too), 1 it
 * reached its budget, 2 + j it matched sequence j; of several matches at one step the lowest j wins, and a sequence wins over the budget.
 * out_tokens[s][k] is 0 for k >= out_len[s].
 * The invariant.  After the call slot s is bit for bit what the matching rwkv_decode_batch_* call with the same n_streams and
 * n_steps = out_len[s] leaves for that slot: its five state arrays, its logits row s and, with penalties, its count vector.  Every
 * returned token but the last has been fed, the last pick has not, and its count is in: a stopped stream is continued by feeding
 * out_tokens[s][out_len[s] - 1].
 * Match history.  The newest RWKV_STOP_MAX_LEN - 1 ids per slot live on the device, one 32-byte record per slot of max_ctx, allocated
 * by the first call that can stop a stream.  Without RWKV_STOP_KEEP a call starts its slots' histories with first_tokens[s]; with it
 * the history continues, unless its newest id is not first_tokens[s] (the caller fed something in between): then it restarts.  So a
 * 16-step call gives exactly the ids, lengths, reasons and final slots of an 8-step call followed by an 8-step KEEP call, a sequence
 * across the boundary included (with nucleus penalties the second call also takes RWKV_NUCLEUS_KEEP and seed + 8).
 * How.  No decode kernel skips a stopped stream -- its row keeps running on its own picks -- so the step at which a stream stops copies
 * its state, logits row and counts into a park buffer, and one launch behind the last step copies every parked stream back
 * (csrc/stop.hip.h).  The park buffer belongs to the context like the other per-call buffers (grown, counted by rwkv_resident_bytes,
 * freed with it): 5 L D f64 + 201 KB per stream, + 201 KB with penalties -- 5.4 MB per stream at 7B (L 32, D 4096), 5.6 MB with penalties.
 * Only a call that can stop a stream (n_seqs > 0 or max_new != NULL) allocates it, launches anything extra -- two small launches per
 * step -- or touches the histories; any other call is the plain loop.
 * Bounded run-ahead.  The host never drains the stream inside the call.  After every block of RWKV_STOP_POLL steps it enqueues an
 * 8-byte copy of the device's count of active streams into a pinned ring, and an event; before enqueuing block b >= 2 it waits for the
 * event of block b - 2 and enqueues nothing more when that word is 0.  The device keeps 8 - 16 steps queued, and a call whose streams
 * have all stopped wastes at most two blocks: *steps_run, the steps enqueued, is at most
 * min(n_steps, RWKV_STOP_POLL * (floor((Lmax - 1) / RWKV_STOP_POLL) + 2)) with Lmax the largest out_len.  The results do not depend on it.
 * Status: RWKV_E_ARG for what the batch calls reject, an unknown kind, a NULL pick, stop or out_len, n_seqs > RWKV_STOP_MAX_SEQS, n_seqs > 0
 * with a NULL seq_ids or seq_len, a seq_len of 0 or above RWKV_STOP_MAX_LEN, a stop id >= 50277, a max_new of 0 or above n_steps, unknown
 * flag bits or reserved != 0; RWKV_E_STATE as for the batch calls.  Every check runs before anything is launched or allocated: a rejected
 * call leaves state, logits, counts and histories as they were.
 * Out of scope: token 0 (<|endoftext|>) is never generated here and so stops nothing -- the greedy pick bans it inside the captured token
 * graph, as every loop above does.
 *
 * rwkv_debug_stop_scan runs the stop test alone over PLANTED picks -- ids is host [n][steps], stream s on slot s and its history, no model
 * step in between, state and logits untouched -- the way the sampler suites plant logits (tests/test_stop_gpu.py). */
#define RWKV_STOP_MAX_SEQS 16u
#define RWKV_STOP_MAX_LEN 8u
#define RWKV_STOP_POLL 8u /* steps per block of the bounded run-ahead */
#define RWKV_STOP_KEEP 1u /* continue the slots' match history from the previous call */
enum rwkv_pick_kind { RWKV_PICK_GREEDY = 0, RWKV_PICK_TYPICAL = 1, RWKV_PICK_NUCLEUS = 2 };
typedef struct rwkv_pick {
    int kind;
    float temp, tau;
    int typical_flags;           /* TYPICAL: as rwkv_decode_batch_typical */
    rwkv_nucleus_params nucleus; /* NUCLEUS: as rwkv_decode_batch_nucleus */
} rwkv_pick;
typedef struct rwkv_stop_params {
    const uint64_t *seq_ids; /* host: the stop sequences, concatenated */
    const uint32_t *seq_len; /* host [n_seqs], each 1 .. RWKV_STOP_MAX_LEN */
    uint32_t n_seqs;         /* 0 .. RWKV_STOP_MAX_SEQS */
    uint32_t flags;          /* RWKV_STOP_KEEP */
    const uint32_t *max_new; /* host [n_streams], each 1 .. n_steps; NULL: n_steps for every stream */
    uint64_t reserved;       /* must be 0 */
} rwkv_stop_params;
int rwkv_decode_batch_until(rwkv_ctx *ctx, const uint64_t *first_tokens, uint64_t n_streams, uint64_t n_steps, const rwkv_pick *pick,
                            const uint64_t *seeds /* NULL for greedy */, const rwkv_stop_params *stop,
                            uint64_t *out_tokens /* [n_streams][n_steps] */, uint32_t *out_len /* [n_streams] */,
                            uint32_t *out_reason /* [n_streams], may be NULL */, uint64_t *steps_run /* may be NULL */);
int rwkv_debug_stop_scan(rwkv_ctx *ctx, const uint64_t *ids /* host [n][steps] */, const uint64_t *first_tokens, uint64_t n, uint64_t steps,
                         const rwkv_stop_params *stop, uint32_t *out_len, uint32_t *out_reason);

/* ---- scoring: how probable is a given token, on the device (no reference counterpart: the reference only generates) ----
 * What they replace is a download: rwkv_forward, rwkv_get_output of [n][50277] f32 logits (201 KB per position) and a log-softmax on
 * the host.  A query is (logits row r, target id g).  With l_i the f32 logits of row r widened to f64, M = max_i l_i, d_i = l_i - M
 * and Z = sum_i exp(d_i):
 *     logprob = d_g - log Z                                      a target whose logit is -inf gives -inf
 *     entropy = log Z - (sum_{i: d_i > -inf} exp(d_i) d_i) / Z   in nats; a -inf logit carries no mass and contributes 0
 *     argmax  = the lowest id with l_i == M                      nothing is banned here: id 0 can win
 * Every sum, exp and log is f64 (csrc/score.hip.h); held to |d logprob| <= 1e-10 and |d entropy| <= 1e-9 against numpy f64 on planted
 * rows by tests/test_score_gpu.py.  With NaN or +inf logits the numbers are unspecified; nothing faults.
 *
 * rwkv_score_rows scores n queries against the logits rows the LAST forward left, the way rwkv_sample_typical samples from them: query i
 * reads row rows[i] and target targets[i] (rows need not be consecutive, ascending or distinct); logprob, entropy and argmax are host
 * arrays [n], entropy and argmax may be NULL.  It changes neither logits nor state.  One upload of rows and targets, one launch
 * sequence over all queries, one download; synchronous on return.  Works on any context that holds a head (whole model or last stage).
 *
 * rwkv_score feeds tokens[0 .. n_tokens) in GPT mode on state slot 0 from the current state; logprob[t] (entropy[t], argmax[t]) is that of
 * targets[t] under the logits that follow tokens[t].  A document doc[0 .. m) is scored with tokens = doc, targets = doc + 1,
 * n_tokens = m - 1.  n_tokens may exceed max_ctx: the call runs exactly the forwards a caller's loop over pieces of max_ctx tokens would
 * (t0 = 0, max_ctx, 2 max_ctx, ...), each through the path rwkv_forward takes for that piece -- the chunk path, token by token at the
 * widths without one, the decode kernels for a last piece of one token -- so the logits are bit-identical to that loop's.  The score
 * launches of a piece sit on the context's stream behind the piece and in front of the next one, which overwrites the rows.  Inside the
 * call there is no host synchronisation and no host <-> device copy but the token-id ring of the chunk path, one upload (targets, and
 * the control blocks of the tokens that run one by one) and one download of the results.  On return state and logits buffer are what
 * the last piece left.  Whole-model contexts only.
 *
 * Scratch (per-query partial tuples, the device arrays of rows, targets and results) belongs to the context: allocated at the first
 * call, grown to the largest n seen, counted by rwkv_resident_bytes, freed by rwkv_free.
 * Status: RWKV_E_ARG for a NULL ctx, rows, tokens, targets or logprob, n == 0 or n > RWKV_MAX_SCORE, a row >= max_ctx, a token or target
 * >= 50277; RWKV_E_STATE when not loaded, for rwkv_score_rows on a context without a head, for rwkv_score on a pipeline-stage context.
 * Every check runs before anything is launched: a rejected call leaves state and logits as they were. */
#define RWKV_MAX_SCORE 65536u
int rwkv_score_rows(rwkv_ctx *ctx, const uint64_t *rows, const uint64_t *targets, uint64_t n,
                    double *logprob, double *entropy, uint64_t *argmax);
int rwkv_score(rwkv_ctx *ctx, const uint64_t *tokens, const uint64_t *targets, uint64_t n_tokens,
               double *logprob, double *entropy, uint64_t *argmax);

/* ---- log-probs and top-n alternatives of generated tokens, on the device (no reference counterpart: the reference only generates) ----
 * What a completion server reports as `logprobs` / `top_logprobs`, and what best-of-n ranks by: what the MODEL thought of a token.  For one f32
 * logits row l (widened to f64), M, Z, logprob_i = (l_i - M) - log Z and the entropy are exactly those of the scoring block above: nothing is
 * banned, no penalty, no temperature -- whichever pick generated the token (greedy with logit 0 banned, typical, nucleus with penalties).  What
 * is reported is the model's distribution, not the sampler's; log-probabilities under the penalised or tempered distribution are out of scope.
 * The top-n of a row: the n ids with the largest f32 logits, in descending logit order, equal logits by ascending id, each with its logprob.
 * Id 0 can appear, as in scoring.  A -inf logit can appear once fewer than n finite ones exist, with logprob -inf.  With NaN or +inf logits
 * the result is unspecified, but every id is below 50277 and nothing faults.
 * One definition on the device (csrc/topn.hip.h calls the score kernels' own slice tuple and fold): the logprob of an id of the top-n, the
 * logprob of a pick and rwkv_score_rows of the same row and id are bitwise equal.  Held to ids equal and |d logprob| <= 1e-10 against numpy
 * f64 on planted rows by tests/test_logprobs_gpu.py.
 *
 * rwkv_topn_rows: the top-n of n logits rows the LAST forward left, as rwkv_score_rows reads them (rows need not be consecutive, ascending or
 * distinct).  ids and logprob are host arrays [n][top_n].  One upload of rows, one launch sequence (two launches), one download; synchronous;
 * works on any context with a head; leaves logits and state alone.  n in 1 .. RWKV_MAX_SCORE, top_n in 1 .. RWKV_MAX_TOPN.
 *
 * rwkv_decode_batch_logprobs is rwkv_decode_batch_until with one more hook: the same picks, kernels, seeds, lengths, reasons and final slots as
 * that call with the same arguments -- or, when stop is NULL or cannot stop a stream, as the matching plain batch call (out_len, which may
 * then be NULL, is n_steps everywhere); n_streams == 1 runs the decode kernels, as there.  Behind step k's pick and in front of the stop test,
 * two launches over rows 0 .. n_streams - 1 read the logits rows and the picks the step just wrote and write step k of a record on the device,
 * nothing else: state, logits rows, counts and histories after the call are bit for bit those of the call without it.  lp->logprob[s][k] is the
 * logprob of pick g_k of stream s under the row it was picked from, lp->entropy[s][k] that row's entropy, lp->top_ids / top_logprob [s][k][.]
 * its top-n.  Every entry with k >= out_len[s] is 0 / 0.0.  No host synchronisation and no host <-> device copy inside the loop beyond what the
 * until call does; one download of the record -- the steps that ran -- behind the last step.  The record belongs to the context like the other
 * per-call buffers (grown to the largest call seen, counted by rwkv_resident_bytes, freed with it): 16 (1 + top_n) bytes per stream and step,
 * plus 8 + 128 (4 + top_n) bytes of scratch per stream.  It is kept on the device for the whole call, hence the bound on
 * n_streams * n_steps * (1 + top_n): 96 streams x 2048 steps x (1 + 20) fits, a longer generation is split into calls with the KEEP flags.
 * Status: RWKV_E_ARG for whatever the until call rejects (but a NULL stop), a NULL lp or lp->logprob, top_n > RWKV_MAX_TOPN, top_ids /
 * top_logprob not NULL exactly when top_n > 0, reserved != 0, a NULL out_len with a non-NULL stop, more than RWKV_MAX_LOGPROB_ENTRIES entries;
 * for rwkv_topn_rows a NULL pointer, n or top_n out of range, a row >= max_ctx.  RWKV_E_STATE as for the batch calls (rwkv_topn_rows: not
 * loaded, or a context without a head).  Every check runs before anything is launched or allocated: a rejected call leaves state, logits,
 * counts, histories and buffers as they were. */
#define RWKV_MAX_TOPN 32u
#define RWKV_MAX_LOGPROB_ENTRIES (1u << 22) /* n_streams * n_steps * (1 + top_n) of one call */
int rwkv_topn_rows(rwkv_ctx *ctx, const uint64_t *rows, uint64_t n, uint32_t top_n, uint64_t *ids /* host [n][top_n] */,
                   double *logprob /* host [n][top_n] */);
typedef struct rwkv_logprob_out {
    uint32_t top_n;      /* 0 .. RWKV_MAX_TOPN; 0: no alternatives */
    uint32_t reserved;   /* must be 0 */
    double *logprob;     /* host [n_streams][n_steps]: log-prob of pick g_k under the row it was picked from */
    double *entropy;     /* host [n_streams][n_steps], may be NULL */
    uint64_t *top_ids;   /* host [n_streams][n_steps][top_n]; NULL exactly when top_n == 0 */
    double *top_logprob; /* the same shape */
} rwkv_logprob_out;
int rwkv_decode_batch_logprobs(rwkv_ctx *ctx, const uint64_t *first_tokens, uint64_t n_streams, uint64_t n_steps, const rwkv_pick *pick,
                               const uint64_t *seeds, const rwkv_stop_params *stop /* may be NULL */, const rwkv_logprob_out *lp,
                               uint64_t *out_tokens, uint32_t *out_len /* may be NULL when stop is NULL */, uint32_t *out_reason,
                               uint64_t *steps_run);

/* ---- beam search on the device: width-W decode with state reordering (no reference counterpart: the reference only samples) ----
 * The decoding mode that keeps the W most probable continuations instead of one.  What it replaces is a caller's loop of rwkv_forward(W, PARRALEL),
 * rwkv_topn_rows, a selection on the host and a reordering of the W state slots through rwkv_get_output / rwkv_set_state (5 L D f64 per slot: 5.2 MB
 * per beam at 7B).  Width W lies in 2 .. RWKV_MAX_BEAM and W <= max_ctx; the chunk path is required, as for every batch call with n_streams >= 2.
 * Start.  Slot 0 holds the prompt's state: the call copies it, device to device, into slots 1 .. W - 1.  first_token is fed to all W rows at step 0.
 * The cumulative scores start at c_0 = 0 and c_j = -inf for j >= 1, so step 0 selects among beam 0's candidates only, without a special case.
 * Step k.  Rows 0 .. W - 1 run one PARRALEL step: the schedule of rwkv_forward(W, PARRALEL) with the same kernels, the ids read on the device.  For
 * a live row j the candidates are (j, i) with i over the W ids of row j with the largest f32 logits other than id 0 (token 0 is banned in every
 * device loop), ordered by descending logit, equal logits by ascending id: the row's top W + 1 of the top-n block above without id 0, or else
 * without its last entry.  A candidate's score is c_j + logprob_j(i), ONE f64 add; logprob is the model's, exactly that of rwkv_score_rows: no ban
 * in the normalisation, no temperature.  An ended row j contributes exactly one candidate: (j, its end token again, c_j, token log-prob 0).  The W
 * best candidates become beams 0 .. W - 1 in that order: descending score, equal scores by ascending parent, then by the row's own candidate order.
 * The beams are therefore always sorted and hypothesis 0 is the best.  Beam m records its parent p_m, token g_m, score c_m and the token's log-prob;
 * it is ended if its parent was ended or if g_m is one of the n_stop <= RWKV_BEAM_MAX_STOP single-token stop ids, and its length is then fixed at
 * k + 1, or at the parent's length.  Slot m receives the five state arrays that slot p_m held after this step, for all m simultaneously, and row m
 * is fed g_m at step k + 1.
 * End.  The tokens are backtracked on the host from the downloaded record: tokens[m][k] is 0 for k >= len[m], token_logprob likewise 0.0, score[m] =
 * c_m.  For a live hypothesis slot m follows the contract of the other loops: every returned token but the last has been fed.  The state of an
 * ended hypothesis's slot is unspecified.  The logits rows are left as the last step wrote them, not permuted.  With NaN or +inf logits the result
 * is unspecified, but every id is below 50277, every parent is below W and nothing faults.
 * Inside the loop there is no host synchronisation and no host <-> device copy: one upload (first_token, stop ids), one download of the record.
 * Per step the call adds five launches to the PARRALEL step: the two top-n launches (n = W + 1), the selection across rows (one workgroup) and the
 * two launches of the state gather (csrc/beam.hip.h).  The buffers belong to the context like the other per-call buffers (grown to the largest
 * call seen, counted by rwkv_resident_bytes, freed with it): the record, 8 (5 W + 16 + 3 W n_steps) bytes; the staging buffer of the gather,
 * 40 W L D bytes (84 MB at 7B and W = 16); the top-n scratch of the log-prob block for W rows and n = W + 1.
 * Out of scope: a length penalty inside the search (the caller ranks score / len^a itself); ending the call early when all beams have ended (it
 * runs n_steps); stop sequences longer than one token; sampling or penalties inside a beam.
 *
 * rwkv_state_permute is the gather on its own: slot m receives what slot parents[m] held at the call, for m = 0 .. n - 1 simultaneously; slots >= n
 * and the logits stay as they are.  Any map works -- identity, swaps, cycles, fan-out: re-fork the survivors of a best-of-n, resample particles.
 * rwkv_debug_beam_step runs ONE selection and state gather on whatever the logits rows 0 .. W - 1 and the state slots hold (planted by the tests, as
 * rwkv_debug_stop_scan plants picks): in cum [W], ended [W], last [W] (the ids the rows were fed: an ended row's end token); out parent [W],
 * token [W], score [W], token_logprob [W], ended_out [W].
 * Status: RWKV_E_ARG for a NULL pointer (token_logprob may be NULL), a width outside 2 .. RWKV_MAX_BEAM or above max_ctx, n_steps == 0 or above
 * RWKV_MAX_DECODE_STEPS, a token or stop id >= 50277 or a stop id of 0, n_stop > RWKV_BEAM_MAX_STOP or > 0 with NULL stop_ids, reserved != 0; for
 * rwkv_state_permute a parent >= n, n == 0 or n > max_ctx.  RWKV_E_STATE when not loaded, on a pipeline-stage context or (rwkv_decode_beam) without the
 * chunk path; rwkv_state_permute needs only a loaded context.  Every check runs before anything is launched or allocated: a rejected call leaves
 * state, logits and buffers as they were. */
#define RWKV_MAX_BEAM 16u
#define RWKV_BEAM_MAX_STOP 16u
typedef struct rwkv_beam_params {
    uint32_t width, n_stop;   /* 2 .. RWKV_MAX_BEAM; 0 .. RWKV_BEAM_MAX_STOP */
    const uint64_t *stop_ids; /* host [n_stop], each 1 .. 50276; may be NULL when n_stop == 0 */
    uint64_t reserved;        /* must be 0 */
} rwkv_beam_params;
typedef struct rwkv_beam_out {
    uint64_t *tokens;      /* host [W][n_steps] */
    uint32_t *len;         /* host [W] */
    double *score;         /* host [W] */
    double *token_logprob; /* host [W][n_steps], may be NULL */
} rwkv_beam_out;
int rwkv_decode_beam(rwkv_ctx *ctx, uint64_t first_token, uint64_t n_steps, const rwkv_beam_params *params, const rwkv_beam_out *out);
int rwkv_state_permute(rwkv_ctx *ctx, const uint32_t *parents, uint64_t n);
int rwkv_debug_beam_step(rwkv_ctx *ctx, const rwkv_beam_params *params, const double *cum, const uint8_t *ended, const uint64_t *last,
                         uint32_t *parent, uint64_t *token, double *score, double *token_logprob, uint8_t *ended_out);

/* ---- constrained decoding on the device: a token automaton and a logit bias (no reference counterpart: the reference only samples) ----
 * The control of a completion API that restricts what may be generated at all: `logit_bias` and banned ids, "answer with one of these strings",
 * JSON / regex / grammar output.  What it replaces is a caller's loop of rwkv_forward, a 201 KB download per stream, a mask on the host, an upload of
 * the row and rwkv_sample_nucleus.  The project has no tokenizer: the caller compiles the regex / grammar / choice list to a token-level automaton
 * with a library of their own and this engine runs it (include/rwkv_sampler.h constraint_trie builds the choice-list case).
 * Automaton.  S states (1 .. RWKV_CONSTRAINT_MAX_STATES) in CSR form: row_ptr u32 [S + 1], tok u32 [nnz], next u32 [nnz], nnz <=
 * RWKV_CONSTRAINT_MAX_EDGES.  The edges of state q are row_ptr[q] .. row_ptr[q + 1]; row_ptr[0] = 0, row_ptr is non-decreasing and row_ptr[S] = nnz;
 * inside a row tok is strictly ascending; every tok lies in 1 .. 50276 (id 0 is never generated by a device loop, so an edge on it is rejected);
 * every next < S.  A state without edges is TERMINAL.  Each state slot owns one automaton state q[max_ctx] (u32 on the device, with a host copy so
 * that checks need no launch).
 * Bias list.  Per stream and sparse: at most RWKV_CONSTRAINT_MAX_BIAS pairs (id strictly ascending, 1 .. 50276; f32 value, finite or -inf: -inf
 * bans the id).
 * Constrained row.  Of logits row l under state q and bias b: c_i = l_i + b_i where q has an edge on i -- ONE f32 add, b_i = 0 where i is not
 * listed -- and c_i = -inf otherwise: i = 0 included, and a listed id that q does not allow too.
 * Constrained pick.  The EXISTING pick run on c instead of l: greedy is k_argmax_rows and its finish (ties to the lowest id, id 0 skipped);
 * nucleus is the three nucleus launches without the ban (the row already holds -inf at id 0); penalties, counts, seeds and u of step k are exactly
 * those of the plain loops.  RWKV_PICK_TYPICAL under a constraint is RWKV_E_ARG.  After pick g the slot advances: q <- next[e] for the edge e of q
 * with tok[e] == g.
 * GUARANTEED: a pick is always an id that q allows (with NaN or +inf logits the pick is unspecified but below 50277, q then stays, and nothing
 * faults); the model's logits buffer is never written -- c lives in a second buffer packed like it -- so the log-probs of the log-prob hook stay
 * the MODEL's; rows, state and counts of an unconstrained call are bit for bit what they are without this block.
 *
 * rwkv_constraint_set validates on the host in O(nnz) (include/rwkv_sampler.h constraint_check is the one validator), uploads the CSR, builds a bit
 * mask [S][1572] u32 on the device (6288 bytes per state; the row of a terminal state allows every id but 0: a row that keeps running behind its
 * stream's end must still pick a valid id, and its picks are discarded) and puts every slot's q to 0; a rejected set leaves the previous automaton
 * installed.  rwkv_constraint_clear removes it (and puts every q to 0).  The CSR, the mask, the second row buffer ([max_ctx][50277] f32, allocated by the
 * first call that needs it) and q belong to the context: counted by rwkv_resident_bytes, freed with it.
 * rwkv_constraint_state_set / _get write and read q[slot0 .. slot0 + n) (set: every state < S; without an automaton only 0).
 * rwkv_pick_constrained is the single draw, as rwkv_sample_nucleus is for the plain sampler: it reads logits row `row` of the LAST forward under
 * q[slot] and `bias` (may be NULL), with slot's counts for penalties (updated only with RWKV_NUCLEUS_UPDATE; RWKV_NUCLEUS_BAN0 changes nothing
 * here), leaves logits and state alone and advances q[slot] only with `advance`; *state_out (may be NULL) is q[slot] on return.
 * rwkv_debug_constrained_row downloads row `row` of the second buffer as the last constrained pick or step left it (tests).
 * rwkv_decode_batch_constrained is rwkv_decode_batch_logprobs with the constraint hook: stream s on slot s starts in start[s] (NULL: in the slot's
 * current q) under its own bias list -- bias_ptr [n_streams + 1] into bias_tok / bias_val; all three NULL for none -- and ends, besides at stop
 * sequences and budgets (stop may be NULL) where its automaton reaches a terminal state: out_reason RWKV_STOP_CONSTRAINT, reported at the call's
 * last step too.  Of several ends at one step a stop sequence (2 + j) wins over the constraint, and the constraint over the budget (1).  lp may
 * be NULL (no record).  out_state (may be NULL) receives q[s].  n_streams == 1 runs the decode kernels, more streams the PARRALEL step, as
 * everywhere else.  Without an installed automaton the call constrains by the bias lists alone: one implicit state that allows every id but 0
 * (start must then be NULL or all 0).
 * The invariant, as for the until call: after the call slot s holds bit for bit what the same call with n_steps = out_len[s] and no stops leaves --
 * the five state arrays, logits row s (the model's), the counts and q[s], the state after consuming out_tokens[s][0 .. out_len[s]).  A
 * constrained call always parks and unparks like a call that can stop a stream.  With the KEEP flags, start = NULL and seed + 8 a 16-step call equals
 * an 8-step call followed by an 8-step call.
 * Inside the loop there is no host synchronisation and no copy beyond what the until call does; per step the call adds two launches
 * (k_constrain_rows: one read of 201 KB + 6.3 KB and one write of 201 KB per row, not a walk over the edges; k_constraint_advance) and one
 * `done` word per stream for k_stop_step; the one-stream greedy loop also runs the row pick's two launches in place of the token graph's pick node.
 * Status: RWKV_E_ARG for whatever the log-prob / until call rejects, a malformed automaton or bias list (each rule above), a start state >= S or
 * terminal (also through a slot's kept state), RWKV_PICK_TYPICAL, reserved != 0; RWKV_E_STATE as for the batch calls.  Every check runs before
 * anything is launched or allocated: a rejected call leaves state, logits, counts, histories, q, the installed automaton and the buffers as they were.
 * Out of scope: beam search under a constraint; typical sampling under a constraint (k_typical_stats forms e * d with d = -inf); log-probs under
 * the constrained distribution; compiling a grammar or regex (the caller brings the automaton); applying the mask inside the pick kernels instead
 * of through a second row. */
#define RWKV_CONSTRAINT_MAX_STATES 4096u
#define RWKV_CONSTRAINT_MAX_EDGES (1u << 24)
#define RWKV_CONSTRAINT_MAX_BIAS 300u
#define RWKV_STOP_CONSTRAINT 32u /* out_reason: the stream's automaton reached a terminal state */
typedef struct rwkv_automaton {
    uint32_t n_states;       /* S: 1 .. RWKV_CONSTRAINT_MAX_STATES */
    uint32_t reserved;       /* must be 0 */
    uint64_t nnz;            /* <= RWKV_CONSTRAINT_MAX_EDGES */
    const uint32_t *row_ptr; /* host [S + 1] */
    const uint32_t *tok;     /* host [nnz]; may be NULL when nnz == 0 */
    const uint32_t *next;    /* host [nnz]; likewise */
} rwkv_automaton;
typedef struct rwkv_bias {
    uint32_t n;          /* 0 .. RWKV_CONSTRAINT_MAX_BIAS */
    uint32_t reserved;   /* must be 0 */
    const uint32_t *tok; /* host [n], strictly ascending, 1 .. 50276 */
    const float *val;    /* host [n], finite or -inf */
} rwkv_bias;
typedef struct rwkv_constrain_params {
    const uint32_t *start;    /* host [n_streams]; NULL: continue from the slots' current q */
    const uint32_t *bias_ptr; /* host [n_streams + 1], bias_ptr[0] = 0, non-decreasing; NULL (with bias_tok and bias_val): no bias */
    const uint32_t *bias_tok; /* host [bias_ptr[n_streams]] */
    const float *bias_val;    /* the same shape */
    uint32_t *out_state;      /* host [n_streams], may be NULL */
    uint64_t reserved;        /* must be 0 */
} rwkv_constrain_params;
int rwkv_constraint_set(rwkv_ctx *ctx, const rwkv_automaton *automaton);
int rwkv_constraint_clear(rwkv_ctx *ctx);
int rwkv_constraint_state_set(rwkv_ctx *ctx, uint64_t slot0, uint64_t n, const uint32_t *states);
int rwkv_constraint_state_get(rwkv_ctx *ctx, uint64_t slot0, uint64_t n, uint32_t *states);
int rwkv_pick_constrained(rwkv_ctx *ctx, uint64_t row, uint64_t slot, const rwkv_pick *pick, const rwkv_bias *bias /* may be NULL */, double u,
                          int advance, uint64_t *token, uint32_t *state_out /* may be NULL */);
int rwkv_debug_constrained_row(rwkv_ctx *ctx, uint64_t row, float *dst /* host [50277] */);
int rwkv_decode_batch_constrained(rwkv_ctx *ctx, const uint64_t *first_tokens, uint64_t n_streams, uint64_t n_steps, const rwkv_pick *pick,
                                  const uint64_t *seeds, const rwkv_constrain_params *constrain, const rwkv_stop_params *stop /* may be NULL */,
                                  const rwkv_logprob_out *lp /* may be NULL */, uint64_t *out_tokens, uint32_t *out_len, uint32_t *out_reason,
                                  uint64_t *steps_run);

/* ---- speculative greedy decoding: a draft verified in one pass of the chunk path (no reference counterpart: the reference decodes token by token) ----
 * One stream, greedy.  rwkv_spec_verify feeds the rows [token, draft[0], .., draft[n_draft - 1]] to slot 0 in ONE GPT-mode pass of the chunk path
 * (n_draft + 1 <= 32 rows, one half: every weight byte is read once for all of them), picks every row as rwkv_decode_greedy picks -- logit 0 is
 * banned, ties go to the lowest id, no winner gives 0 -- and keeps the longest prefix of the draft that the picks confirm:
 *     a = the number of leading i with draft[i] == pick[i]                (row i's pick is the id that follows token, draft[0 .. i - 1])
 * On return slot 0 holds the state after rows 0 .. a, i.e. after the a + 1 ids token, draft[0 .. a - 1] were fed; *n_accepted = a; *next_token =
 * pick[a], which has been emitted but not fed, as with rwkv_decode_greedy: feed it as the next call's `token`.  Logits rows 0 .. n_draft are what
 * rwkv_forward of the same rows leaves.  The pass commits nothing itself: it leaves every row's state in a checkpoint buffer
 * (4 L (n_draft + 1) n_embed f64, the context's, allocated at the first call for the largest n_draft seen: 134 MB at 7B for 31), a one-wave kernel
 * finds a, and a copy kernel writes xy, aa, bb, dd of slot 0 from checkpoint row a (pp is not touched: the chunk path does not use it).  There is
 * no host synchronisation between the pass and the commit; the call waits once, for 16 bytes.  n_draft == 0 is a plain one-token step on the
 * chunk path (draft may then be NULL).  Slots >= 1, the penalty counts and the constraint states are not touched.
 * THE VERIFIER IS THE CHUNK PATH, not the decode kernels rwkv_decode_greedy runs.  The two paths compute the same logits to within the project's
 * parity bound (held to 3e-5 of the row's largest |logit|; about 3e-6 measured), so the ids equal rwkv_decode_greedy's wherever the top two logits
 * of a row lie further apart than the two paths differ; in an exact near-tie the ids may differ, and both results are within the parity contract.
 * What is exact: the result does not depend on the draft -- the state, the logits rows 0 .. a and the ids are bit for bit those of
 * rwkv_forward(rows 0 .. a) for a >= 1, and of rwkv_spec_verify(n_draft = 0) for a = 0.
 * Status: RWKV_E_ARG for a NULL output pointer (or NULL draft with n_draft > 0), n_draft > RWKV_SPEC_MAX_DRAFT or n_draft + 1 > max_ctx, any id >=
 * 50277; RWKV_E_STATE when not loaded, on a pipeline-stage context, or without the chunk path (the rule of rwkv_decode_batch_greedy with n_streams
 * >= 2).  Every check runs before any launch: a rejected call leaves the state and the logits as they were.
 *
 * rwkv_decode_speculative is the loop around it with a draft MODEL: draft_ctx is a second whole-model context on the same device, usually a smaller
 * model.  On entry both contexts hold the same prefix in slot 0; on return both have consumed first_token, out_tokens[0 .. n_tokens - 2], so calls
 * chain: feed out_tokens[n_tokens - 1] as the next first_token.  Per round, with k' = min(k, remaining - 1):
 *     1. the draft model runs k' + 1 greedy steps on its slot 0 with its decode kernels and copies slot 0 into slot i + 1 behind step i
 *        (so draft_ctx needs max_ctx >= k + 2; its slots 1 .. k + 1 are scratch of the call);
 *     2. the target verifies the k' drafts (rwkv_spec_verify without its wait in front of the download);
 *     3. the draft's slot 0 is restored from its slot a + 1;
 *     4. a + 1 ids are emitted: draft[0 .. a - 1], next.
 * A call never emits or consumes more than n_tokens.  At most two host synchronisations per round, each with a download of a few bytes (the drafts;
 * {a, next}); no logits leave the device.  At the end the logits row the last id was picked from is copied to row 0.  out_tokens does not depend on
 * the draft model at all: it is the continuation that repeated rwkv_spec_verify(n_draft = 0) gives, whatever the draft guesses -- the draft only
 * decides how many rounds that takes.  The comparison with rwkv_decode_greedy is the one above: THE VERIFIER IS THE CHUNK PATH; ids equal wherever
 * the top two logits lie further apart than the two paths differ (held to 3e-5, about 3e-6 measured), and may differ in an exact near-tie, both
 * within the parity contract.  stats (may be NULL): rounds, ids drafted (sum of k'), ids accepted (sum of a).
 * Status: as rwkv_spec_verify for ctx; RWKV_E_ARG also for k == 0, k > RWKV_SPEC_MAX_DRAFT, draft_ctx == ctx or NULL, a draft context on another
 * device or with max_ctx < k + 2, ctx with max_ctx < k + 1, n_tokens == 0 or above RWKV_MAX_DECODE_STEPS; RWKV_E_STATE for a draft context that is
 * not loaded or is a pipeline stage.
 * Out of scope: sampled acceptance (rejection sampling needs the draft's probabilities), draft trees, more than one stream, pipeline contexts,
 * drafts longer than one half. */
#define RWKV_SPEC_MAX_DRAFT 31u
int rwkv_spec_verify(rwkv_ctx *ctx, uint64_t token, const uint64_t *draft, uint64_t n_draft, uint64_t *n_accepted, uint64_t *next_token);
typedef struct rwkv_spec_stats {
    uint64_t rounds, drafted, accepted;
} rwkv_spec_stats;
int rwkv_decode_speculative(rwkv_ctx *ctx, rwkv_ctx *draft_ctx, uint64_t first_token, uint64_t n_tokens, uint32_t k, uint64_t *out_tokens,
                            rwkv_spec_stats *stats /* may be NULL */);

/* ---- segmented forward: many sequences of any length behind one read of the weights (no reference counterpart: the reference has the two ends) ----
 * The rows of a call are SEGMENTS: segment i is n consecutive tokens of the sequence on state slot `slot`, and the segments' tokens stand back to
 * back in `tokens`.  One segment {0, n} is rwkv_forward's GPT mode, n segments of length 1 are its PARRALEL mode, and a mix is the step of a
 * continuous-batching server: the decoding streams' last picks and a piece of every waiting prompt, admitted on their own slots, in one call.
 * Row numbering and logits: T = sum n; row j of the call is token j of the packed array and its logits land in row j of the device logits buffer,
 * where rwkv_score_rows, rwkv_topn_rows and rwkv_sample_nucleus(row, slot) read them.  last_row[i] (may be NULL) is the row of segment i's last
 * token, the one a server picks from.
 * Arguments: 1 <= T <= max_ctx, n_segs >= 1, every n >= 1, every slot < max_ctx, THE SLOTS OF ONE CALL ARE PAIRWISE DISTINCT, every id < 50277,
 * flags == 0.
 * State: segment i starts from what slot segs[i].slot holds and leaves that slot after its n tokens (xy, aa, bb, dd; pp is untouched, as
 * everywhere on the chunk path).  Slots not named, the penalty counts, the stop histories and the constraint states are untouched.
 * Every call runs the CHUNK PATH, T == 1 included (the one-row pass that rwkv_spec_verify(n_draft = 0) is).  The rows are cut into passes exactly
 * as rwkv_forward cuts them -- 32 rows for T <= 32 or RWKV_SEQ_ROWS=32, else 64 in two halves -- and more than one pass runs the RWKV_SEQ_STAGES
 * pipeline.  A segment may straddle a half or a pass boundary: the piece behind a pass boundary continues from the slot, which the piece in front
 * of it has just written on the same stage's stream.  Synchronous on return, like rwkv_forward; inside the call the row plan is uploaded once and
 * the ids once per pass through the pinned ring, and there is no host synchronisation between passes.  At the first call the context allocates the
 * plan (8 max_ctx bytes) and 64 n_embed f64 of staging per pipeline stage in use; rwkv_resident_bytes counts them.
 * EXACT: the result for a segment does not depend on what else is in the call or where its rows sit -- its slot's state and its logits rows are
 * bit for bit those of the same segment alone in a call.  A single segment {0, n}, n >= 2, leaves state and logits rows 0 .. n - 1 bit for bit as
 * rwkv_forward(tokens, n, RWKV_MODE_GPT) does, and {0, 1} as rwkv_spec_verify(token, NULL, 0, ..) does.  Against rwkv_forward(RWKV_MODE_PARRALEL)
 * for segments of length 1 the results lie within the chunk path's parity bounds; bit equality there is not promised (DESIGN.md has what was
 * measured): the PARRALEL kernels leave roundings to the compiler that the GPT walk pins.
 * Status: RWKV_E_ARG for each rule above and for a NULL ctx, tokens or segs; RWKV_E_STATE when not loaded, on a pipeline-stage context, or without
 * the chunk path (the rule of rwkv_decode_batch_greedy with n_streams >= 2).  Every check runs before anything is launched or allocated: a rejected
 * call leaves state, logits and buffers as they were.
 *
 * rwkv_segment_plan is the ONE validator (rwkv_forward_segments calls it) and needs neither a context nor a device: it checks a segment list
 * against max_ctx by the rules above (the ids aside) and writes the per-row plan the device reads: row_slot[j], the slot of row j; row_flags[j],
 * bit 0 set when the row is the first of its piece (its shift input and WKV state come from the slot), bit 1 when it is the last of its piece (its
 * LayerNorm outputs and WKV state go to the slot).  A piece ends where its segment ends or where the pass ends, so the plan depends on the pass
 * size: the exported function assumes passes of 64 rows (rwkv_forward_segments plans for the pass size it runs).  row_slot, row_flags and n_rows
 * may each be NULL (validate only); nothing is written when the list is rejected.
 * Out of scope: a device-side decode loop with admission, a batched sampler over arbitrary (row, slot) pairs (rwkv_sample_nucleus is one call per
 * stream), logits for the last rows only, segments on pipeline-stage contexts, the same slot twice in one call, checkpointing (speculative)
 * segments. */
typedef struct rwkv_segment { uint32_t slot; uint32_t n; } rwkv_segment;   /* n >= 1 consecutive tokens of the sequence on state slot `slot` */
int rwkv_forward_segments(rwkv_ctx *ctx, const uint64_t *tokens /* [T], the segments' tokens back to back */,
                          const rwkv_segment *segs, uint64_t n_segs, uint32_t flags /* must be 0 */,
                          uint64_t *last_row /* host [n_segs], may be NULL: logits row of each segment's last token */);
int rwkv_segment_plan(const rwkv_segment *segs, uint64_t n_segs, uint64_t max_ctx,
                      uint32_t *row_slot /* [T] */, uint8_t *row_flags /* [T], may both be NULL: validate only */, uint64_t *n_rows);

/* ---- layer pipeline (no reference counterpart: the reference is single-device) ----
 * A context may own a contiguous layer range [l0, l1) of the model: call rwkv_set_layer_range()
 * before loading.  The first stage (l0 == 0) also owns the embedding table + ln0, the last stage
 * (l1 == n_layers) ln_out + head.  rwkv_stage_forward() runs this stage's share of ONE token on
 * state slot `slot`: stage 0 starts from `token`; later stages start from the residual vector the
 * caller has placed in rwkv_x_device() (f64[n_embed], e.g. by an RCCL recv) and leave their output
 * there for the next hop.  On the last stage `pick` (may be NULL) receives the greedy id. */
int rwkv_set_layer_range(rwkv_ctx *ctx, uint64_t l0, uint64_t l1);
int rwkv_stage_forward(rwkv_ctx *ctx, uint64_t token, uint32_t slot, uint64_t *pick);
double *rwkv_x_device(rwkv_ctx *ctx);

/* One prompt chunk (n <= 64 consecutive tokens of one sequence, GPT mode: one weight pass, two 32-row halves above 32) through THIS stage's layers on the mm8_seq /
 * MFMA path.  The chunk's residual stream [n][n_embed] f64 lives in buffer `buf` (0 or 1) of the context
 * (rwkv_xseq_device): stage 0 fills it from `tokens`, a later stage expects the previous stage's output there and leaves
 * its own in it; the last stage also writes the logits rows [row0, row0 + n).  Asynchronous (rwkv_sync to wait). */
int rwkv_stage_chunk(rwkv_ctx *ctx, const uint64_t *tokens, uint64_t n, uint64_t row0, int buf);
double *rwkv_xseq_device(rwkv_ctx *ctx, int buf);
/* Same-device hand-over of a chunk's residual stream between two stage contexts (several stages per GPU, tests). */
int rwkv_xseq_copy(rwkv_ctx *dst, int dst_buf, rwkv_ctx *src, int src_buf, uint64_t rows);
int rwkv_sync(rwkv_ctx *ctx);

/* ---- native transport of the pipeline: RCCL send/recv over xGMI, enqueued on the engine's own stream ----
 * (north_star: "layers optionally pipeline across the 8 GPUs of one node via RCCL send/recv over xGMI").  One process
 * per GPU; rank r's context holds layers [l0_r, l1_r) (rwkv_set_layer_range before loading), rank 0 the embedding, the
 * last rank the head.  librccl.so is resolved at run time by the first of these calls, so single-GPU users never load it.
 *   rwkv_pipe_rccl_path  which RCCL these calls bind in this process (path of the shared object holding ncclSend; loads it if
 *                        need be, no GPU involved).  Order: RWKV_RCCL_LIB if set; else the copy the process has ALREADY loaded (a
 *                        PyTorch-ROCm host carries torch/lib/librccl.so, built against the HIP runtime torch brought along --
 *                        the engine's streams live in that runtime too); else the system's librccl.so.1
 *   rwkv_pipe_unique_id  one rank makes the 128-byte communicator id (ncclGetUniqueId) and distributes it out of band
 *   rwkv_pipe_init       every rank joins (ncclCommInitRank); the rank must match the context's layer range.  The ranks then AGREE,
 *                        over the communicator, on the prefill micro-batch (64 or 32 rows: RWKV_SEQ_ROWS and max_ctx are per-rank
 *                        values) and on n_embed / n_layers / world; a mismatch fails every rank with RWKV_E_ARG.  One line describing
 *                        this rank's end of the transport goes to stderr
 *   rwkv_pipe_info       that description as a JSON object: rank, world, layer range, device ordinal, PCI bus id, arch, RCCL version
 *                        code + path of the shared object holding ncclSend, HIP runtime version, agreed prefill rows
 *   rwkv_pipe_decode     greedy decode of `world` independent streams (one per stage in flight, state slot = stream),
 *                        n_steps tokens each; first_tokens[world] is read on rank 0, picks[world][n_steps] written on
 *                        the last rank.  The hop (f64[n_embed] forward, the picked id u64 back to rank 0) and the stage
 *                        graph alternate on one stream; the host does not wait inside the loop
 *   rwkv_pipe_decode_streams   the same with only the first n_streams (1..world) streams' slots of the schedule filled:
 *                        n_streams = 1 is ONE stream through all the stages -- the latency of single-stream decode on
 *                        the pipeline, t_tok + (world - 1) hops + the fed-back id; picks stays [world][n_steps]
 *   rwkv_pipe_profile / rwkv_pipe_hop_stats   hop timing: event pairs around the per-tick RCCL group of the last
 *                        rwkv_pipe_decode* call; out4 = {ticks measured, mean, min, max microseconds} (min = the hop
 *                        itself, the peer's data was waiting; the mean includes waiting for the peer)
 *   rwkv_pipe_prefill    RWKV::loadContext (rwkv.h:395-413) across the stages: the prompt's 64-token passes (32 with max_ctx < 64 or RWKV_SEQ_ROWS=32) are the
 *                        micro-batches, stage s works on chunk t - s at tick t; needs max_ctx >= 32; tokens read on rank 0 */
int rwkv_pipe_rccl_path(char *out, uint64_t cap);
int rwkv_pipe_unique_id(void *out128);
int rwkv_pipe_init(rwkv_ctx *ctx, const void *id128, int rank, int world);
int rwkv_pipe_info(rwkv_ctx *ctx, char *out, uint64_t cap);
int rwkv_pipe_decode(rwkv_ctx *ctx, const uint64_t *first_tokens, uint64_t n_steps, uint64_t *picks);
int rwkv_pipe_decode_streams(rwkv_ctx *ctx, const uint64_t *first_tokens, uint64_t n_steps, uint64_t n_streams, uint64_t *picks);
/* 2 x world streams in flight on TWO communicators (the second one is created at the first call, its id travels over the first): the
 * streams of even and odd index run the tick schedule above on their own communicator and HIP stream, the stage alternates between
 * them on the engine's stream -- one parity's hop is in flight while the stage works on the other's item (a tick costs
 * max(t_stage, t_hop) instead of their sum).  first_tokens[2 * world] (rank 0), picks[2 * world][n_steps] (last rank); needs
 * max_ctx >= 2 * world state slots.  Every rank of the pipeline must call it. */
int rwkv_pipe_decode_dual(rwkv_ctx *ctx, const uint64_t *first_tokens, uint64_t n_steps, uint64_t *picks);
int rwkv_pipe_profile(rwkv_ctx *ctx, int on);
int rwkv_pipe_hop_stats(rwkv_ctx *ctx, double *out4);
int rwkv_pipe_prefill(rwkv_ctx *ctx, const uint64_t *tokens, uint64_t n_tokens);
void rwkv_pipe_free(rwkv_ctx *ctx);

/* Replaces freeTensors(), rwkv.cu:719-730, plus destruction of the handle. */
void rwkv_free(rwkv_ctx *ctx);

const char *rwkv_last_error(void);

/* ---- introspection / measurement hooks (no reference counterpart) ---- */

/* Device pointer behind slot `slot` of the reference's RWKV::tensors[] table (rwkv.h:248; slots: enums/enum.h:7-55)
 * where the engine keeps that tensor in FILE layout: the f32/f64 vectors, the five state arrays, X and BUFFER2 (logits).
 * NULL for the uint8 matrices (re-tiled at load) and for pure scratch.  EMBED is a device pointer here (the reference
 * keeps the table on the host, rwkv.cu:683-684). */
void *rwkv_tensor_device(rwkv_ctx *ctx, int slot);
/* Device pointer of the logits buffer ([max_ctx][50277] f32). */
float *rwkv_logits_device(rwkv_ctx *ctx);
/* Device pointer of a state array ([max_ctx][L][D] f64), rwkv_state_id. */
double *rwkv_state_device(rwkv_ctx *ctx, int which);
/* The HIP stream (hipStream_t) all engine work is enqueued on. */
void *rwkv_stream(rwkv_ctx *ctx);
/* Device bytes this context holds: decode-layout weights + row sums + site tables + embedding + state + scratch and, when
 * max_ctx > 1 on a whole-model context, the SECOND resident copy of the matrices in the MFMA B-operand image of the chunk
 * path (+7.2 GB at 7B, +13.9 GB at 14B). */
uint64_t rwkv_resident_bytes(const rwkv_ctx *ctx);
/* The decode form of a loaded context: which of the four per-layer decode kernel classes stream the tile image (csrc/tile.hip.h,
 * DESIGN.md 4.7), bit 0 K/V/R + WKV, bit 1 att_out, bit 2 ffn k/r, bit 3 ffn_v; a clear bit = that class runs the register row
 * form (csrc/kernels.hip.h).  A class's matrices are resident in the one layout its kernel streams (on 256 CUs: 15 at 4096 and
 * 5120 channels, 13 at 2048, 0 otherwise; RWKV_TILE=<mask> before the load overrides).  -1 without a loaded model. */
int rwkv_decode_form(const rwkv_ctx *ctx);
/* Algorithmic HBM bytes of one token (13*L*D^2 + V*D uint8 weight bytes
 * + 168*L*D + 40*D bytes of vectors/state). */
uint64_t rwkv_bytes_per_token(const rwkv_ctx *ctx);

/* Per-kernel-class device time of the last rwkv_profile_token() call, measured with HIP events
 * on the engine's stream.  Classes: 0 embed+ln0, 1 att K/V/R+wkv, 2 att_out, 3 ffn r+k,
 * 4 ffn_v, 5 head, 6 argmax.  ms[c] = total milliseconds over `reps` tokens, bytes[c] =
 * algorithmic uint8 weight bytes of one launch of that class, launches[c] = launches/token. */
#define RWKV_N_KCLASS 7
int rwkv_profile_token(rwkv_ctx *ctx, uint64_t token, int reps, double *ms, uint64_t *bytes,
                       uint32_t *launches);

/* Like rwkv_profile_token, but ONE event pair brackets a batch of `reps` x (launches per token) back-to-back
 * launches of each class, so the per-launch figure is not inflated by per-bracket event overhead and is
 * comparable with rocprofv3 kernel durations.  ms[c] = total ms of the batch, n[c] = launches in it.
 * Leaves the recurrent state zeroed (the batches run the kernels out of token order). */
int rwkv_profile_batched(rwkv_ctx *ctx, uint64_t token, int reps, double *ms, uint32_t *n);

/* Tuning aid: run one eager token with phase timestamps enabled in the middle layer's ffn r+k
 * kernel; out receives grid*8*8 stamps of the 100 MHz device wall clock ([workgroup][wave][phase]). */
int rwkv_debug_timeline(rwkv_ctx *ctx, uint64_t token, unsigned long long *out, uint64_t cap);

/* ---- per-kernel parity hooks: the production decode kernels one launch at a time ----
 * rwkv_debug_launch runs ONE launch of decode kernel class `cls` -- 0 k_first (embedding + ln0, rwkv.cu:513-524; opens the first ln1
 * site), 1 k_att (ln1, mixatt, mm8_threec, wkv_forward: rwkv.cu:535-545), 2 k_attout (mm8_one att_out + residual, :548-553),
 * 3 k_ffn_rk (ln2, mixffn, mm8_one ffn_r + sigmoid, mm8_one ffn_k + relu^2, :557-573), 4 k_ffnv (mm8_one<float> ffn_v + blockout,
 * :574-577), 5 k_head (ln_out + mm8_one head, :585-589), 6 the greedy pick -- of layer `layer`, eagerly, in the form (row / tile) the
 * context runs that class in, on whatever its buffers hold, and waits for it.  cls 0 also sets the token's control block (token id, state
 * slot); the other classes take the slot from the last cls-0 call.  A token is 0, then 1..4 per layer, then 5: the launches of the
 * captured token graph, one at a time, so that a test can read every hand-over between two kernels and check each kernel against the
 * oracle's piece for it on that kernel's OWN inputs (tests/test_kernels_gpu.py).
 * rwkv_debug_read / rwkv_debug_write copy an intermediate vector of the decode path to / from host memory (sizes in bytes; n_embed = D,
 * grid = rwkv_debug_grid() workgroups per launch). */
enum rwkv_debug_buf {
    RWKV_DBG_X = 0,        /* f64[D]     residual stream */
    RWKV_DBG_YBUF = 1,     /* f32[D]     k_att -> k_attout: gated wkv output (rwkv.cu:250, cast to f32 as :290 does) times att_out's scale r[j] */
    RWKV_DBG_PART_ATT = 2, /* f64[grid]  k_att -> k_attout: per-workgroup partial sums of (gated wkv) * att_out's offset o[j] */
    RWKV_DBG_PMAX_ATT = 3, /* f32[grid]  k_att -> k_attout: per-workgroup max |YBUF| */
    RWKV_DBG_HBUF = 4,     /* f32[4 D]   k_ffn_rk -> k_ffnv: relu(k)^2 (rwkv.cu:189-190) times ffn_v's scale r[j] */
    RWKV_DBG_RGATE = 5,    /* f32[D]     k_ffn_rk -> k_ffnv: sigmoid(r) (rwkv.cu:212) */
    RWKV_DBG_PART_FFN = 6, /* f64[grid]  k_ffn_rk -> k_ffnv: per-workgroup partial sums of relu(k)^2 * ffn_v's offset o[j] */
    RWKV_DBG_PMAX_FFN = 7, /* f32[grid]  k_ffn_rk -> k_ffnv: per-workgroup max |HBUF| */
    RWKV_DBG_LNSTAT = 8    /* f64[3][2]  mean, rstd of the last ln1 / ln2 / ln_out site */
};
int rwkv_debug_launch(rwkv_ctx *ctx, int cls, uint64_t layer, uint64_t token, uint32_t slot);
int rwkv_debug_read(rwkv_ctx *ctx, int which, void *dst, uint64_t cap_bytes);
int rwkv_debug_write(rwkv_ctx *ctx, int which, const void *src, uint64_t bytes);
uint64_t rwkv_debug_grid(const rwkv_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* RWKV_MI355X_H */
