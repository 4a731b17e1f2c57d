// score.hip.h -- log-probability, entropy and argmax of logits rows ON THE DEVICE (gfx950): what a caller needs to score a text
// (perplexity, the log-likelihood of each answer of a multiple-choice item, re-ranking) without downloading 201 KB of logits per position.
// No reference counterpart: the reference only generates.
//
// A query is (logits row r, target id g).  With l_i the f32 logits of row r widened to f64, M = max_i l_i, d_i = l_i - M and
// Z = sum_i exp(d_i):
//     logprob = d_g - log Z                                       (a target whose logit is -inf: -inf)
//     entropy = log Z - (sum_{i: d_i > -inf} exp(d_i) d_i) / Z    (nats; a -inf logit carries no mass and adds 0, never 0 * inf)
//     argmax  = the lowest id with l_i == M                       (nothing is banned: this is scoring, id 0 can win)
// Every sum, exp and log is f64, as in the sampler.  NaN or +inf logits give unspecified numbers; no index leaves the vocabulary.
//
// Two launches cover all queries of a call, the query on blockIdx.y:
//   k_score_part    (SC_G, n) workgroups: workgroup (b, q) holds slice b of the row of query q in registers (one dword load per
//                   element: a row starts 4 r bytes past a 16-byte boundary and V is odd, so nothing here depends on alignment) and
//                   writes the tuple (m, z = sum exp(l - m), s = sum exp(l - m) (l - m), lowest id at m) of its slice
//   k_score_finish  one wave per query: folds the SC_G tuples (the sampler's ts_combine with the -inf guards), reads the target's logit
// The row of a query comes from a device array: rows need not be consecutive or distinct.
#pragma once
#include "kernels.hip.h"

namespace rwkvk {

constexpr int SC_G = 16;                   // workgroups (slices of the vocabulary) per query
constexpr int SC_NT = 256;                 // threads of k_score_part
constexpr int SC_PER = (((int)VOCAB + SC_G - 1) / SC_G + SC_NT - 1) / SC_NT;   // elements per thread: the longest slice fits the registers of a workgroup
constexpr size_t SC_PART_Q = (size_t)SC_G * 4;   // doubles of `part` per query
constexpr unsigned SC_MAX_Y = 65535u;      // queries per launch (gridDim.y)
static_assert(SC_G <= 64, "one lane per partial in the finish");
static_assert(SC_NT * SC_PER >= ((int)VOCAB + SC_G - 1) / SC_G, "score tiling must cover the longest slice (k_score_part is launched with SC_G slices)");

struct ScoreArgs {
    const float *logits;                   // [rows][V]
    const unsigned long long *rows;        // [n] logits row of query q (checked on the host: < max_ctx)
    const unsigned long long *targets;     // [n] target id of query q (checked on the host: < V)
    double *part;                          // [n][SC_G][4] (m, z, s, id)
    double *logprob, *entropy;             // [n]
    unsigned long long *argmax;            // [n]
};

// The tuple of one slice, and the slice itself: workgroup (b, .) loads slice b of the row `lg` into v (one dword per element; behind the slice: -inf)
// and returns the slice's first id.  Every thread ends with the slice maximum `best` and the lowest id `besti` that holds it, thread 0 with
// z = sum exp(l - best) and s = sum exp(l - best) (l - best) over the slice.  k_score_part and the top-n part kernel (topn.hip.h) both call this:
// one way of summing, so one log-probability on the device.
__device__ __forceinline__ int score_slice(const float *lg, float (&v)[SC_PER], float &best, unsigned &besti, double &tz, double &ts)
{
    __shared__ float sv[SC_NT / 64];
    __shared__ unsigned si[SC_NT / 64];
    __shared__ double red[2 * (SC_NT / 64)];
    const int V = (int)VOCAB;
    const int i0 = block_lo(V), i1 = block_hi(V);
#pragma unroll
    for (int k = 0; k < SC_PER; k++) {       // all SC_PER loads in flight; behind the slice: -inf, which neither wins nor carries mass
        const int i = i0 + (int)threadIdx.x + k * SC_NT;
        v[k] = i < i1 ? lg[i] : -INFINITY;
    }
    // slice maximum and the lowest id that holds it ((value, id) fold of the greedy pick: wave_max is for non-negative values)
    best = -INFINITY;
    besti = 0xffffffffu;
#pragma unroll
    for (int k = 0; k < SC_PER; k++)
        if (v[k] > best) { best = v[k]; besti = (unsigned)(i0 + (int)threadIdx.x + k * SC_NT); }
    am_wave_fold(best, besti);
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = best; si[threadIdx.x >> 6] = besti; }
    __syncthreads();
    best = sv[0]; besti = si[0];
#pragma unroll
    for (int w = 1; w < SC_NT / 64; w++)
        if (am_better(sv[w], si[w], best, besti)) { best = sv[w]; besti = si[w]; }
    const double m = (double)best;
    double z = 0.0, s = 0.0;
#pragma unroll
    for (int k = 0; k < SC_PER; k++) {
        const bool mass = v[k] > -INFINITY;                      // (a slice of -inf only: m = -inf, nothing has mass, z = s = 0)
        const double d = mass ? (double)v[k] - m : 0.0;
        const double e = mass ? exp(d) : 0.0;
        z += e; s += e * d;
    }
    z = wave_sum(z); s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) { red[(threadIdx.x >> 6) * 2] = z; red[(threadIdx.x >> 6) * 2 + 1] = s; }
    __syncthreads();
    tz = 0.0; ts = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < SC_NT / 64; w++) { tz += red[2 * w]; ts += red[2 * w + 1]; }
    return i0;
}

__global__ __launch_bounds__(SC_NT) void k_score_part(ScoreArgs a)
{
    float v[SC_PER], best;
    unsigned besti;
    double tz, ts;
    score_slice(a.logits + (size_t)a.rows[blockIdx.y] * VOCAB, v, best, besti, tz, ts);
    if (threadIdx.x == 0) {
        double *part = a.part + blockIdx.y * SC_PART_Q + blockIdx.x * 4;
        part[0] = (double)best; part[1] = tz; part[2] = ts; part[3] = (double)besti;
    }
}

// The fold of one row's SC_G tuples on one wave (the sampler's ts_combine with the -inf guards): every lane ends with M = mm, Z, S = sum exp(d) d
// and `at`, the lowest id that holds M.  k_score_finish and the top-n finish (topn.hip.h) both call this.
__device__ __forceinline__ void score_fold(const double *row_part, int lane, double &mm, double &Z, double &S, unsigned &at)
{
    const double *part = row_part + (lane < SC_G ? lane : 0) * 4;
    const bool on = lane < SC_G;
    const double m = on ? part[0] : -INFINITY, z = on ? part[1] : 0.0, s = on ? part[2] : 0.0;
    at = on ? (unsigned)part[3] : 0xffffffffu;
    mm = m;
    for (int off = 32; off >= 1; off >>= 1) mm = fmax(mm, __shfl_xor(mm, off, 64));
    // a slice without mass (m = -inf) adds nothing: not exp(-inf) * (-inf * 0)
    const bool mass = on && m > -INFINITY;
    const double sc = mass ? exp(m - mm) : 0.0;
    Z = wave_sum(sc * z); S = wave_sum(mass ? sc * (s + (m - mm) * z) : 0.0);
    if (!(on && m == mm)) at = 0xffffffffu;                      // the lowest id among the slices that hold the maximum
    for (int off = 32; off >= 1; off >>= 1) at = min(at, (unsigned)__shfl_xor((int)at, off, 64));
}

__global__ __launch_bounds__(64) void k_score_finish(ScoreArgs a)
{
    const int lane = threadIdx.x;
    const unsigned q = blockIdx.x;
    double mm, Z, S;
    unsigned at;
    score_fold(a.part + q * SC_PART_Q, lane, mm, Z, S, at);
    const double logZ = log(Z);
    if (lane == 0) {
        const double lt = (double)a.logits[(size_t)a.rows[q] * VOCAB + a.targets[q]];
        a.logprob[q] = (lt - mm) - logZ;
        if (a.entropy) a.entropy[q] = logZ - S / Z;
        if (a.argmax) a.argmax[q] = at < VOCAB ? at : 0u;        // no winner (all NaN or all -inf): 0, as the greedy pick
    }
}

} // namespace rwkvk
