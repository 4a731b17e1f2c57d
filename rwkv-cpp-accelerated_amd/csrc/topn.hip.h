// topn.hip.h -- the n most probable ids of logits rows, with their log-probabilities, ON THE DEVICE (gfx950, wave64): what a completion server
// reports as `logprobs` / `top_logprobs` of a generated token, without downloading 201 KB of logits per stream and step.
// No reference counterpart: the reference only generates.
//
// For one f32 logits row l, M, Z, logprob_i = (l_i - M) - log Z and the entropy are those of score.hip.h -- not restated here but CALLED:
// k_topn_part runs score_slice, k_topn_finish runs score_fold, the same 16 slices in the same order, and a log-probability is formed by the
// one expression k_score_finish uses.  The log-prob of an id of the top-n, of a pick and of rwkv_score_rows on the same row and id are the same bits.
// The top-n of a row: the n ids with the largest f32 logits, descending, equal logits by ascending id.  Nothing is banned (id 0 can appear), a
// -inf logit can appear once fewer than n finite ones exist (logprob -inf); with NaN or +inf logits the result is unspecified, every id is
// below VOCAB and nothing faults.
//
// Order.  An element is the 64-bit key (order-preserving 32-bit image of its f32 logit) << 32 | (2^32 - 1 - id): a larger key is a better
// element, the keys of a row are distinct, and one unsigned compare is the whole rule -- larger logit first, then lower id.  (-0.0 is keyed as
// +0.0: they are equal logits.)  Key 0 is no element: it fills the places behind a slice's end and loses against every element.
//
// Two launches cover all rows of a call or step, the row on blockIdx.y / blockIdx.x as in the score kernels:
//   k_topn_part    (SC_G, rows) workgroups of SC_NT threads: workgroup (b, q) holds slice b of row q in registers (score_slice: 13 dwords per
//                  thread, single-dword loads -- a row starts 4 r bytes past a 16-byte boundary and V is odd), writes the slice's score tuple
//                  and selects the slice's best n on those registers.  Each WAVE takes its own best n in n rounds of a 64-lane fold of the key
//                  (no barrier inside: a round is 13 compares and six cross-lane steps; all n may lie in one thread's registers, a taken
//                  element is masked, not overwritten, so a -inf logit stays a candidate); the four sorted lists of a workgroup meet in LDS,
//                  where thread (w, r) counts the keys above its own -- its rank among the 4 n -- and the n best leave in order
//   k_topn_finish  one workgroup per row, one thread per candidate (16 n <= 512): every wave folds the 16 tuples (score_fold: same bits in every
//                  wave), every thread ranks its candidate among the 16 n in LDS, and the n best write id and log-prob at their rank.  Thread 0
//                  also writes the log-prob of the row's pick and the entropy when the caller records them (the device decode loops)
// The kernel is latency-bound on one small row: what it costs is the n dependent fold rounds of the part kernel (profiles/NOTES.md).
#pragma once
#include "score.hip.h"

namespace rwkvk {

constexpr unsigned TOPN_MAX = 32u;                        // RWKV_MAX_TOPN
constexpr unsigned TOPN_FINISH_NT = SC_G * TOPN_MAX;      // threads of k_topn_finish at most: one per candidate
static_assert(TOPN_FINISH_NT <= 1024, "one thread per candidate in the finish");
static_assert(SC_PER <= 32, "one bit per register in the taken mask");
// every wave of k_topn_part holds at least TOPN_MAX elements of the shortest slice: its lists are never short of real elements
static_assert(((int)VOCAB / SC_G / SC_NT) * 64 >= (int)TOPN_MAX, "a wave's share of a slice holds n elements");

struct TopnArgs {
    const float *logits;                   // [rows][V]
    const unsigned long long *rows;        // [R] logits row of query q (checked on the host: < max_ctx); nullptr: query q reads row q
    const unsigned long long *picks;       // [R] the id whose log-prob is recorded with query q (device loops); nullptr: none
    double *part;                          // [R][SC_G][4] score tuples
    unsigned long long *cand;              // [R][SC_G][n] the best n keys of each slice, descending
    unsigned n;                            // 0 .. TOPN_MAX
    unsigned long long *ids;               // [R][n]
    double *logprob;                       // [R][n]
    double *pick_logprob, *entropy;        // [R], with picks
};

// order-preserving image of an f32: a < b as floats <=> key(a) < key(b) as unsigned (NaNs land at the two ends)
__device__ __forceinline__ unsigned topn_key32(float v)
{
    const unsigned b = v == 0.f ? 0u : __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ unsigned long long topn_key(float v, unsigned id) { return ((unsigned long long)topn_key32(v) << 32) | (0xffffffffu - id); }
__device__ __forceinline__ unsigned topn_id(unsigned long long key)
{
    const unsigned id = 0xffffffffu - (unsigned)(key & 0xffffffffull);
    return id < VOCAB ? id : 0u;           // (key 0, or a word nothing wrote: no index leaves the vocabulary)
}
// every lane ends with the largest key of the wave
__device__ __forceinline__ unsigned long long topn_wave_max(unsigned long long k)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(k >> 32), m, 64), lo = (unsigned)__shfl_xor((int)(unsigned)k, m, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        if (o > k) k = o;
    }
    return k;
}
// rank of list entry `at` (key `mine`) among `lists` sorted lists of n keys each, list j at sc[j * stride ...]: how many entries are better.  Equal keys
// (only key 0 repeats) rank by position, so the ranks are a permutation
__device__ __forceinline__ unsigned topn_rank(const unsigned long long *sc, unsigned lists, unsigned stride, unsigned n, unsigned long long mine, unsigned at)
{
    unsigned rank = 0;
    for (unsigned j = 0; j < lists; j++)
        for (unsigned r = 0; r < n; r++) {
            const unsigned long long o = sc[j * stride + r];
            rank += (o > mine || (o == mine && j * stride + r < at)) ? 1u : 0u;
        }
    return rank;
}

__global__ __launch_bounds__(SC_NT) void k_topn_part(TopnArgs a)
{
    constexpr unsigned NW = SC_NT / 64;
    __shared__ unsigned long long sc[NW * TOPN_MAX];
    const unsigned q = blockIdx.y;
    float v[SC_PER], best;
    unsigned besti;
    double tz, ts;
    const int i0 = score_slice(a.logits + (size_t)(a.rows ? a.rows[q] : q) * VOCAB, v, best, besti, tz, ts);
    if (threadIdx.x == 0) {
        double *part = a.part + q * SC_PART_Q + blockIdx.x * 4;
        part[0] = (double)best; part[1] = tz; part[2] = ts; part[3] = (double)besti;
    }
    const unsigned n = a.n;
    if (n == 0) return;                                        // (the whole grid: log-prob and entropy only)
    const int i1 = block_hi((int)VOCAB);
    unsigned long long key[SC_PER];
#pragma unroll
    for (int k = 0; k < SC_PER; k++) {
        const int i = i0 + (int)threadIdx.x + k * SC_NT;
        key[k] = i < i1 ? topn_key(v[k], (unsigned)i) : 0ull;
    }
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned taken = 0u;
    for (unsigned r = 0; r < n; r++) {                         // the wave's r-th best: no barrier, the four waves run their rounds independently
        unsigned long long lb = 0ull;
        unsigned lk = 0u;
#pragma unroll
        for (int k = 0; k < SC_PER; k++) {
            const unsigned long long kk = ((taken >> k) & 1u) ? 0ull : key[k];
            if (kk > lb) { lb = kk; lk = (unsigned)k; }
        }
        const unsigned long long wb = topn_wave_max(lb);
        if (wb != 0ull && lb == wb) taken |= 1u << lk;         // the keys are distinct: one lane holds it
        if (lane == 0) sc[wave * TOPN_MAX + r] = wb;
    }
    __syncthreads();
    if (threadIdx.x < NW * TOPN_MAX && (threadIdx.x & (TOPN_MAX - 1)) < n) {
        const unsigned long long mine = sc[threadIdx.x];
        const unsigned rank = topn_rank(sc, NW, TOPN_MAX, n, mine, threadIdx.x);
        if (rank < n) a.cand[((size_t)q * SC_G + blockIdx.x) * n + rank] = mine;
    }
}

// launched with 64 * ceil(SC_G n / 64) threads (64 for n = 0)
__global__ __launch_bounds__(TOPN_FINISH_NT) void k_topn_finish(TopnArgs a)
{
    __shared__ unsigned long long sc[SC_G * TOPN_MAX];
    const unsigned q = blockIdx.x, n = a.n, C = SC_G * n;
    double mm, Z, S;
    unsigned at;
    score_fold(a.part + q * SC_PART_Q, (int)(threadIdx.x & 63), mm, Z, S, at);
    const double logZ = log(Z);
    const float *lg = a.logits + (size_t)(a.rows ? a.rows[q] : q) * VOCAB;
    if (threadIdx.x == 0 && a.picks) {
        const unsigned long long g = a.picks[q];
        const double lt = (double)lg[g < VOCAB ? g : 0ull];
        a.pick_logprob[q] = (lt - mm) - logZ;
        a.entropy[q] = logZ - S / Z;
    }
    if (threadIdx.x < C) sc[threadIdx.x] = a.cand[(size_t)q * C + threadIdx.x];
    __syncthreads();
    if (threadIdx.x < C) {
        const unsigned long long mine = sc[threadIdx.x];
        const unsigned rank = topn_rank(sc, SC_G, n, n, mine, threadIdx.x);
        if (rank < n) {
            const unsigned id = topn_id(mine);
            const double lt = (double)lg[id];
            a.ids[(size_t)q * n + rank] = id;
            a.logprob[(size_t)q * n + rank] = (lt - mm) - logZ;
        }
    }
}

} // namespace rwkvk
