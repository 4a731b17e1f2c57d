// stop.hip.h -- stop sequences and per-stream token budgets for the device decode loops (gfx950); include/rwkv_mi355x.h
// rwkv_decode_batch_until has the contract, include/rwkv_sampler.h stop_scan is the same scan on the host.
//
// No decode or chunk kernel knows about stopping: the chunk path maps row t to slot slot0 + t and the decode kernels update the state in
// place, so a stopped stream cannot be skipped.  Its row keeps running on its own picks (valid ids), and what it had when it stopped is
// set aside:
//     k_stop_step   behind each step's pick, one thread per stream: append the pick to the slot's match history, test every stop sequence
//                   against the newest ids, the constraint's `done` word and the budget; on a hit record length and reason and lower the
//                   count of active streams
//     k_stop_park   grid (chunks, streams): a stream that stopped THIS step copies its five state arrays, its logits row and, with
//                   penalties, its count vector into the park buffer; every other workgroup exits at once
//     unpark        k_stop_park<true>, once behind the last enqueued step: every stopped stream is copied back, so the slot is what it
//                   was at the stop whatever ran afterwards (the same kernel with the copy turned round)
// The match history of a stopped stream is not touched again (k_stop_step skips the stream), so it needs no parking.
// Plain C++ and vector memory operations only; nothing here writes host memory or waits for anything.  The host reads the active count
// through an asynchronous copy every RWKV_STOP_POLL steps (engine.hip Stopper).
#pragma once
#include "kernels.hip.h"

namespace rwkvk {

constexpr int STOP_MAX_SEQS = 16, STOP_MAX_LEN = 8;
constexpr int STOP_HIST = 8;                   // u32 per slot: the newest STOP_MAX_LEN - 1 ids, newest first, and one word of padding (32 bytes)
constexpr unsigned STOP_NONE = 0xFFFFFFFFu;    // an empty history entry (no token id)
constexpr unsigned STOP_CONSTRAINT = 32u;      // RWKV_STOP_CONSTRAINT: the reason of a stream whose automaton reached a terminal state
constexpr int STOP_NT = 64;                    // threads per workgroup of k_stop_step
constexpr int PARK_NT = 256, PARK_CHUNKS = 32; // k_stop_park: workgroups per stream
constexpr size_t PARK_ROW = (VOCAB + 3 + 3) / 4 * 4;    // floats of a parked logits row or count vector: the row behind the source's offset inside 16 bytes

// the stop sequences, passed by value with every launch (580 bytes)
struct StopTable {
    unsigned n_seqs;
    unsigned len[STOP_MAX_SEQS];
    unsigned ids[STOP_MAX_SEQS][STOP_MAX_LEN];     // ids[j][i]: the i-th id of sequence j counted from its END (newest first, as the history)
};

struct StopArgs {
    StopTable t;
    unsigned n;                          // streams; stream s = slot s
    unsigned n_steps;                    // of the call: a budget equal to it is no stop
    int keep;                            // RWKV_STOP_KEEP
    unsigned *hist;                      // [max_ctx][STOP_HIST]
    unsigned long long *active;          // streams that have not stopped
    const unsigned long long *first;     // [n] the first tokens
    unsigned *len, *reason;              // [n] 0 until the stream stops
    const unsigned *max_new;             // [n]
    const unsigned *done;                // [n] constrained decoding (constrain.hip.h): the stream's automaton reached a terminal state at this step; nullptr: none
};

// picks: [n] the ids picked at step k.  At step 0 the history (re)starts from the first token unless it continues (keep) from that very id.
__global__ __launch_bounds__(STOP_NT) void k_stop_step(const StopArgs a, const unsigned long long *__restrict__ picks, unsigned k)
{
    const unsigned s = blockIdx.x * STOP_NT + threadIdx.x;
    if (s >= a.n) return;
    if (a.len[s]) return;
    unsigned *h = a.hist + (size_t)s * STOP_HIST;
    unsigned w[STOP_MAX_LEN];            // the newest ids, newest first
    w[0] = (unsigned)picks[s];
#pragma unroll
    for (int i = 1; i < STOP_MAX_LEN; i++) w[i] = h[i - 1];
    if (k == 0) {
        const unsigned f = (unsigned)a.first[s];
        if (!a.keep || w[1] != f) {
            w[1] = f;
#pragma unroll
            for (int i = 2; i < STOP_MAX_LEN; i++) w[i] = STOP_NONE;
        }
    }
    unsigned reason = 0;
    for (unsigned j = 0; j < a.t.n_seqs && !reason; j++) {
        bool hit = true;
#pragma unroll
        for (int i = 0; i < STOP_MAX_LEN; i++) hit = hit && (i >= (int)a.t.len[j] || w[i] == a.t.ids[j][i]);
        if (hit) reason = 2 + j;
    }
    if (!reason && a.done && a.done[s]) reason = STOP_CONSTRAINT;       // behind the sequences, in front of the budget; reported at the call's last step too
    if (!reason && k + 1 == a.max_new[s] && k + 1 < a.n_steps) reason = 1;
#pragma unroll
    for (int i = 0; i < STOP_MAX_LEN - 1; i++) h[i] = w[i];
    if (reason) {
        a.len[s] = k + 1;
        a.reason[s] = reason;
        atomicAdd(a.active, ~0ull);      // - 1
    }
}

struct ParkArgs {
    double *state[5];                    // [max_ctx][LD]
    float *logits;                       // [max_ctx][V]
    float *counts;                       // [max_ctx][V], nullptr without penalties
    float *park;                         // per stream: 5 x LD f64 | PARK_ROW f32 logits | PARK_ROW f32 counts (with penalties)
    size_t LD;                           // L * D, a multiple of 16
    size_t stride;                       // floats per parked stream
    const unsigned *len;                 // [n]
};

// this workgroup's share of n floats; dst and src sit at the SAME offset inside 16 bytes: single floats up to the boundary, 16-byte vectors
// behind it, single floats for the rest
__device__ __forceinline__ void stop_copy(float *__restrict__ dst, const float *__restrict__ src, size_t n)
{
    const size_t tid = (size_t)blockIdx.x * PARK_NT + threadIdx.x, nt = (size_t)gridDim.x * PARK_NT;
    size_t head = ((16 - (reinterpret_cast<uintptr_t>(src) & 15)) & 15) / 4;
    if (head > n) head = n;
    const size_t body = (n - head) / 4, done = head + 4 * body;
    if (tid < head) dst[tid] = src[tid];
    uint4 *d4 = reinterpret_cast<uint4 *>(dst + head);
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src + head);
    for (size_t i = tid; i < body; i += nt) d4[i] = s4[i];
    if (tid < n - done) dst[done + tid] = src[done + tid];
}

// step1 = k + 1 of the step just picked: the streams with len == step1 are parked; UNPARK: every stream with len != 0 is copied back
template <bool UNPARK> __global__ __launch_bounds__(PARK_NT) void k_stop_park(const ParkArgs a, unsigned step1)
{
    const unsigned s = blockIdx.y, l = a.len[s];
    if (UNPARK ? l == 0 : l != step1) return;
    float *p = a.park + (size_t)s * a.stride;
    for (int i = 0; i < 5; i++) {
        float *live = reinterpret_cast<float *>(a.state[i] + (size_t)s * a.LD);
        if (UNPARK) stop_copy(live, p, 2 * a.LD); else stop_copy(p, live, 2 * a.LD);
        p += 2 * a.LD;
    }
    for (int i = 0; i < (a.counts ? 2 : 1); i++) {
        float *live = (i ? a.counts : a.logits) + (size_t)s * VOCAB;
        float *q = p + ((reinterpret_cast<uintptr_t>(live) >> 2) & 3);
        if (UNPARK) stop_copy(live, q, VOCAB); else stop_copy(q, live, VOCAB);
        p += PARK_ROW;
    }
}

} // namespace rwkvk
