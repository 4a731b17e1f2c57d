// beam.hip.h -- beam search ON THE DEVICE (gfx950, wave64): the selection of the W best continuations across the W rows of a step, and the
// simultaneous gather of the recurrent state that follows it.  include/rwkv_mi355x.h rwkv_decode_beam has the contract, include/rwkv_sampler.h
// beam_select is the same selection on the host.  No reference counterpart: the reference only samples.
//
// What a step of the search needs of a logits row is its W + 1 best ids with their log-probabilities, and those are the top-n kernels' own
// output (topn.hip.h, launched unchanged with n = W + 1): nothing of a row is read here.
//     k_beam_select   ONE workgroup behind the two top-n launches, one thread per candidate (row j, place i of its top W + 1), at most 16 x 17.
//                     A live row offers its W best ids other than id 0 (id 0 is dropped where it is among the W + 1, else the last entry is),
//                     each at cum[j] + logprob -- one f64 add; an ended row offers its end token again at cum[j], log-prob 0.  The score's
//                     order-preserving 64-bit image is ranked in LDS by counting (the topn_rank pattern): larger score first, equal scores
//                     by ascending parent, then by the row's own order -- which is the candidate's index, so the ranks are a permutation
//                     whatever the scores are (NaN included).  The W winners write the step's record, the ids of the next step where the
//                     embedding of the chunk path reads them, the new cum / ended / len and the parent map of the gather
//     k_beam_gather   grid (beams, chunks) -- the beams on x: rwkv_state_permute takes up to max_ctx of them -- two launches in the style of
//                     k_stop_park: <false> beam m with parent[m] != m copies the five
//                     state arrays of slot parent[m] into staging slot m, <true> copies them on into slot m; a beam that keeps its slot
//                     exits at once.  Every slot is read before any slot is written, so any map works: swaps, cycles, fan-out.  16-byte
//                     loads and stores, four in flight per thread (L D is a multiple of 16: an array of a slot is a multiple of 128 bytes)
// Plain C++ and vector memory operations only; nothing here writes host memory or waits for anything.
#pragma once
#include "topn.hip.h"

namespace rwkvk {

constexpr unsigned BEAM_MAX = 16u, BEAM_MAX_STOP = 16u;        // RWKV_MAX_BEAM, RWKV_BEAM_MAX_STOP
constexpr unsigned BEAM_CAND = BEAM_MAX * (BEAM_MAX + 1);      // candidates at most
constexpr unsigned BEAM_NT = (BEAM_CAND + 63u) / 64u * 64u;    // threads of k_beam_select at most
constexpr int GATHER_NT = 256, GATHER_CHUNKS_MAX = 128, GATHER_PER = 8;   // k_beam_gather: workgroups per beam at most, 16-byte words per thread aimed at
static_assert(BEAM_MAX + 1 <= TOPN_MAX, "a row's W + 1 candidates are one top-n");

struct BeamArgs {
    unsigned W, n_stop, k;                 // width, stop ids, step
    const unsigned long long *stop;        // [n_stop] single-token stop ids
    const unsigned long long *top_ids;     // [W][W + 1] the rows' top-n (k_topn_finish)
    const double *top_lp;                  // [W][W + 1]
    const unsigned long long *cur;         // [W] the ids the step was fed: an ended row's end token
    unsigned long long *next;              // [W] the ids of the next step
    double *cum;                           // [W] cumulative scores, in and out
    unsigned *ended, *len;                 // [W] in and out
    unsigned *parent;                      // [W] the map of the gather
    unsigned *rec_parent, *rec_token;      // [W] the step's record
    double *rec_score, *rec_lp;            // [W]
};

// order-preserving image of an f64: a < b as doubles <=> key(a) < key(b) as unsigned; -0.0 is keyed as +0.0 (equal scores), NaNs land at the ends
__device__ __forceinline__ unsigned long long beam_key(double v)
{
    const unsigned long long b = v == 0.0 ? 0ull : (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// launched with 64 * ceil(W (W + 1) / 64) threads.  A template (NT = BEAM_NT is its one instance) so that hipcc emits it where the host code first
// names it, behind every kernel of the decode and chunk paths, like the gather: a plain kernel comes out in the order of the headers, in front of
// the template instances of kernels.hip.h / tile.hip.h / seq.hip.h, and moves every one of them in the code object (the single-stream decode
// measured 5 us per token slower that way: profiles/beam/bench_ab.txt)
template <unsigned NT> __global__ __launch_bounds__(NT) void k_beam_select(const BeamArgs a)
{
    __shared__ unsigned long long key[BEAM_CAND];
    __shared__ unsigned char valid[BEAM_CAND];
    const unsigned W = a.W, n = W + 1, C = W * n, t = threadIdx.x;
    const unsigned j = t / n, i = t - j * n;
    bool ok = false, row_ended = false;
    unsigned id = 0, row_len = 0;
    double score = 0.0, lp = 0.0;
    if (t < C) {
        const double cj = a.cum[j];
        row_ended = a.ended[j] != 0u;
        row_len = a.len[j];
        if (row_ended) {                   // exactly one candidate: the end token again, at the row's score
            ok = i == 0;
            const unsigned long long e = a.cur[j];
            id = e < VOCAB ? (unsigned)e : 0u;
            score = cj; lp = 0.0;
        } else {
            const unsigned long long *ids = a.top_ids + (size_t)j * n;
            bool has0 = false;
            for (unsigned r = 0; r < n; r++) has0 = has0 || ids[r] == 0ull;
            const unsigned long long g = ids[i];
            id = g < VOCAB ? (unsigned)g : 0u;
            ok = g != 0ull && (has0 || i < W);
            lp = a.top_lp[(size_t)j * n + i];
            score = cj + lp;
        }
        key[t] = beam_key(score);
        valid[t] = ok ? 1 : 0;
    }
    __syncthreads();                       // every read of cum / ended / len / cur is done: the winners may write
    if (!ok) return;
    const unsigned long long mine = key[t];
    unsigned rank = 0;
    for (unsigned o = 0; o < C; o++) {
        const unsigned long long k = key[o];
        rank += (valid[o] && (k > mine || (k == mine && o < t))) ? 1u : 0u;
    }
    if (rank >= W) return;
    bool stop = false;
    for (unsigned s = 0; s < a.n_stop; s++) stop = stop || a.stop[s] == (unsigned long long)id;
    a.rec_parent[rank] = j; a.rec_token[rank] = id; a.rec_score[rank] = score; a.rec_lp[rank] = lp;
    a.next[rank] = id;
    a.cum[rank] = score;
    a.ended[rank] = (row_ended || stop) ? 1u : 0u;
    a.len[rank] = row_ended ? row_len : a.k + 1u;
    a.parent[rank] = j;
}

struct GatherArgs {
    double *state[5];                      // [max_ctx][LD]
    double *stage;                         // [n][5][LD]
    const unsigned *parent;                // [n]
    unsigned n;
    size_t LD;                             // L * D, a multiple of 16
};

// BACK false: staging slot m <- slot parent[m]; true: slot m <- staging slot m
template <bool BACK> __global__ __launch_bounds__(GATHER_NT) void k_beam_gather(const GatherArgs a)
{
    const unsigned m = blockIdx.x, p = a.parent[m];
    if (p == m || p >= a.n) return;        // (a parent outside the map: checked on the host, never written by the selection)
    const size_t per = a.LD / 2, total = 5 * per;              // 16-byte words of one array, of a slot
    const size_t nt = (size_t)gridDim.y * GATHER_NT;
    uint4 *stage = reinterpret_cast<uint4 *>(a.stage + (size_t)m * 5 * a.LD);
    for (size_t w0 = (size_t)blockIdx.y * GATHER_NT + threadIdx.x; w0 < total; w0 += 4 * nt) {
        uint4 v[4];
        uint4 *dst[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const size_t w = w0 + (size_t)u * nt;
            dst[u] = nullptr;
            if (w < total) {
                const size_t arr = w / per, off = w - arr * per;
                uint4 *live = reinterpret_cast<uint4 *>(a.state[arr] + (size_t)(BACK ? m : p) * a.LD) + off;
                v[u] = BACK ? stage[w] : *live;
                dst[u] = BACK ? live : stage + w;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (dst[u]) *dst[u] = v[u];
    }
}

} // namespace rwkvk
