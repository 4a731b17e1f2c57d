// ratio.hip.h -- the RATIO pick of speculative sampling ON THE DEVICE (gfx950, wave64): a draft MODEL that samples proposes id x from its own
// distribution q; the target accepts it with probability min(1, p(x) / q(x)) and otherwise draws from the normalised max(p - q, 0), which leaves
// the output distributed exactly as p.  include/rwkv_mi355x.h rwkv_spec_ratio_rows has the contract.  No reference counterpart.
//
// The one pick of this project that reads TWO logits rows: l, row q.row of the target's logits buffer, and m, row q.qrow of the draft model's
// logits (any device buffer: another context's logits, or the stash the sampled speculative loop keeps).  Id 0 is banned on both sides, as in
// every device loop.  All arithmetic is f64, in log space:
//     s_i = (double)l_i * inv_tt       M = max_{i >= 1} s_i      Z = sum_{i >= 1} exp(s_i - M)      lp(i) = (s_i - M) - log Z       (lq from m alike)
//     accept iff 1 <= x < V and log(u_a) < lp(x) - lq(x); the pick is then x
//     else r(i) = max(exp(lp(i)) - exp(lq(i)), 0) for i >= 1, i != x; R = sum r; the pick is the smallest i with sum_{i' <= i} r(i') > u_r R
//     R == 0 (both rows peaked on x so sharply that everything else underflows): the largest l_i over i != 0, x; ties to the lowest id
//     x == RT_NONE (the bonus row behind a draft that stands entirely): q = 0 and no accept test, i.e. a draw from p in id order
// ONE launch: one workgroup of 1024 threads per row, rows in blockIdx.y.  Wave w owns ids [3200 w, 3200 w + 3200) as 50 GROUPS of 64 consecutive
// ids, lane j of the wave id 3200 w + 64 k + j of group k: every load of a sweep is one coalesced 256-byte request per row, and the order of the
// ids is (wave, group, lane).  The rows are 201 KB each and were written by the launch in front, so the three sweeps read them from L2 / MALL; a
// thread keeps nothing of them (100 values per thread beside the f64 exponential's registers do not fit the 128 VGPRs a 1024-thread workgroup
// leaves a wave; the resource line is in profiles/spec_ratio/isa_compare.txt).
//     sweep 1   the two f32 maxima (a positive scale keeps the order): DPP in the wave, LDS across the 16 waves
//     sweep 2   the two f64 exp-sums, the same way; then the accept test, uniform over the workgroup: an accepted row ends here
//     sweep 3   r per id; per group the wave's sum T[w][k] (DPP) into LDS, per wave their sum W[w]
//     pick      every thread adds the 16 W in order -> R, the target u_r R and the wave that owns it; that wave walks its 50 T to the group, forms
//               r again there (the same expression, so the same bits), scans it over the lanes and takes the first lane behind the target.
//               Where the orders of summation disagree by a rounding at an edge, the last id with r > 0 in front of it (ts_draw's rule)
// No matrix instruction fits this work.  Plain C++ and vector memory operations only; the kernel writes out[] and acc[] and nothing else.
#pragma once
#include "pickrows.hip.h"

namespace rwkvk {

constexpr int RT_NT = 1024, RT_WAVES = RT_NT / 64;
constexpr int RT_GROUPS = 50;                              // groups of 64 ids per wave
constexpr int RT_WAVE_IDS = RT_GROUPS * 64;                // 3200
constexpr unsigned RT_NONE = 0xffffffffu;                  // no draft id: the bonus row
constexpr unsigned RT_MAX_ROWS = 32u;                      // rows of one launch: one half of a pass
static_assert(RT_WAVES * RT_WAVE_IDS >= (int)VOCAB, "the waves' ids cover the vocabulary");

// One row of a call, as the host fills it
struct RatioQ {
    unsigned row;                 // logits row of the target
    unsigned qrow;                // row of the draft's logits (not read on a bonus row)
    unsigned x;                   // the draft id, or RT_NONE
    unsigned out;                 // out[q.out], acc[q.out]
    double u_a, u_r;              // uniforms in [0, 1): acceptance, draw from the residual
};
static_assert(sizeof(RatioQ) == 32, "the row record is 32 bytes on both sides of the upload");

struct RatioArgs {
    const RatioQ *q;              // [rows of the launch]
    const float *logits;          // the target's [max_ctx][V]
    const float *qlogits;         // the draft's [n][V]; nullptr when every row is a bonus row
    double inv_tt, inv_td;        // 1 / temp_target, 1 / temp_draft (exactly 1 for a temperature of 1)
    unsigned long long *out;      // the picks
    unsigned char *acc;           // 1 where the draft id was accepted
};

// the workgroup's fold of K values per thread through `red[RT_WAVES][K]`; every thread returns with the K totals, folded in wave order
template <int K, class T, class Fold, class WaveFold>
__device__ __forceinline__ void rt_block_fold(T (&v)[K], T *red, WaveFold wave_fold, Fold fold)
{
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = wave_fold(v[k]);
    __syncthreads();              // previous readers of `red` are done
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) red[w * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) {
        T s = red[k];
        for (int i = 1; i < RT_WAVES; i++) s = fold(s, red[i * K + k]);
        v[k] = s;
    }
}

// the id of (wave, group, lane), and whether it is one the pick can return: below V, not 0
__device__ __forceinline__ int rt_id(int w, int k, int lane) { return w * RT_WAVE_IDS + k * 64 + lane; }
__device__ __forceinline__ bool rt_real(int i) { return i >= 1 && i < (int)VOCAB; }

// r(i) of the header, from the two logits of id i; `bonus`: q = 0
__device__ __forceinline__ double rt_resid(float l, float m, bool bonus, double inv_tt, double inv_td, double Mp, double Mq, double logZp, double logZq)
{
    const double ep = exp(((double)l * inv_tt - Mp) - logZp);
    if (bonus) return ep;
    const double d = ep - exp(((double)m * inv_td - Mq) - logZq);
    return d > 0.0 ? d : 0.0;     // (NaN gives 0)
}

template <int NT> __global__ __launch_bounds__(NT) void k_ratio_pick(const RatioArgs a)
{
    static_assert(NT == RT_NT, "sixteen waves, fifty groups each");
    __shared__ double red[RT_WAVES * 2];
    __shared__ double T[RT_WAVES][RT_GROUPS];
    __shared__ double W[RT_WAVES];
    __shared__ float bv[RT_WAVES];
    __shared__ unsigned bi[RT_WAVES];
    const RatioQ q = a.q[blockIdx.y];
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;      // (the wave's number, in a scalar register)
    const bool bonus = q.x == RT_NONE;
    const float *l = a.logits + (size_t)q.row * VOCAB;
    const float *m = bonus ? l : a.qlogits + (size_t)q.qrow * VOCAB;      // (a bonus row never uses what it reads through m)
    const double inv_tt = a.inv_tt, inv_td = a.inv_td;

    // sweep 1: the maxima over the real ids
    float mx[2] = {-INFINITY, -INFINITY};
#pragma unroll 5
    for (int k = 0; k < RT_GROUPS; k++) {
        const int i = rt_id(w, k, lane);
        if (rt_real(i)) { mx[0] = fmaxf(mx[0], l[i]); mx[1] = fmaxf(mx[1], m[i]); }
    }
    rt_block_fold<2>(mx, reinterpret_cast<float *>(red), [](float v) { return wave_max(v); }, [](float x, float y) { return fmaxf(x, y); });
    const double Mp = (double)mx[0] * inv_tt, Mq = (double)mx[1] * inv_td;

    // sweep 2: the exp-sums
    double z[2] = {0.0, 0.0};
#pragma unroll 1
    for (int k = 0; k < RT_GROUPS; k++) {
        const int i = rt_id(w, k, lane);
        if (rt_real(i)) {
            z[0] += exp((double)l[i] * inv_tt - Mp);
            if (!bonus) z[1] += exp((double)m[i] * inv_td - Mq);
        }
    }
    rt_block_fold<2>(z, red, [](double v) { return wave_sum(v); }, [](double x, double y) { return x + y; });
    const double logZp = log(z[0]), logZq = bonus ? 0.0 : log(z[1]);

    // the accept test (uniform over the workgroup: x is below V or RT_NONE, so l[x] and m[x] are inside the rows)
    const bool tested = q.x >= 1u && q.x < VOCAB;
    if (tested) {
        const double lpx = ((double)l[q.x] * inv_tt - Mp) - logZp, lqx = ((double)m[q.x] * inv_td - Mq) - logZq;
        if (log(q.u_a) < lpx - lqx) {
            if (threadIdx.x == 0) { a.out[q.out] = q.x; if (a.acc) a.acc[q.out] = 1; }
            return;
        }
    }

    // sweep 3: the residual's group sums and wave sums
    double ws = 0.0;
#pragma unroll 1
    for (int k = 0; k < RT_GROUPS; k++) {
        const int i = rt_id(w, k, lane);
        double r = 0.0;
        if (rt_real(i) && (unsigned)i != q.x) r = rt_resid(l[i], m[i], bonus, inv_tt, inv_td, Mp, Mq, logZp, logZq);
        const double t = wave_sum(r);
        if (lane == 0) T[w][k] = t;
        ws += t;
    }
    if (lane == 0) W[w] = ws;
    __syncthreads();
    double R = 0.0;
    for (int i = 0; i < RT_WAVES; i++) R += W[i];

    if (!(R > 0.0)) {
        // (uniform over the workgroup) nothing left of the residual in f64: the largest l over the ids other than 0 and x, lowest id first
        float best = -INFINITY;
        unsigned besti = RT_NONE;
#pragma unroll 5
        for (int k = 0; k < RT_GROUPS; k++) {
            const int i = rt_id(w, k, lane);
            if (rt_real(i) && (unsigned)i != q.x && am_better(l[i], (unsigned)i, best, besti)) { best = l[i]; besti = (unsigned)i; }
        }
        am_wave_fold(best, besti);
        if (lane == 0) { bv[w] = best; bi[w] = besti; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int i = 1; i < RT_WAVES; i++)
                if (am_better(bv[i], bi[i], best, besti)) { best = bv[i]; besti = bi[i]; }
            if (besti >= VOCAB) besti = q.x == 1u ? 2u : 1u;      // no winner (logits that are no numbers): an id that is neither 0 nor x
            a.out[q.out] = besti;
            if (a.acc) a.acc[q.out] = 0;
        }
        return;
    }

    // the wave that owns the target: the first whose running total passes it (the last one with mass where a rounding leaves none)
    const double target = q.u_r * R;
    int ow = -1, lastw = 0;
    double c = 0.0, cb = 0.0, lastc = 0.0;
    for (int i = 0; i < RT_WAVES; i++) {
        const double n = c + W[i];
        if (W[i] > 0.0) { lastw = i; lastc = c; }
        if (ow < 0 && n > target) { ow = i; cb = c; }
        c = n;
    }
    if (ow < 0) { ow = lastw; cb = lastc; }
    if (w != ow) return;          // (no barrier from here on)

    // its group, by the same rule
    int kk = -1, lastk = 0;
    c = cb; lastc = cb;
#pragma unroll 1
    for (int k = 0; k < RT_GROUPS; k++) {
        const double t = T[w][k], n = c + t;
        if (t > 0.0) { lastk = k; lastc = c; }
        if (kk < 0 && n > target) { kk = k; cb = c; }
        c = n;
    }
    if (kk < 0) { kk = lastk; cb = lastc; }

    // the id inside the group: r again, an inclusive scan over the lanes, the first lane behind the target
    const int i = rt_id(w, kk, lane);
    double r = 0.0;
    if (rt_real(i) && (unsigned)i != q.x) r = rt_resid(l[i], m[i], bonus, inv_tt, inv_td, Mp, Mq, logZp, logZq);
    double incl = r;
    for (int off = 1; off < 64; off <<= 1) {
        const double v = __shfl_up(incl, off, 64);
        if (lane >= off) incl += v;
    }
    const unsigned long long hit = __ballot(r > 0.0 && cb + incl > target), nz = __ballot(r > 0.0);
    // (nz != 0: the group's sum is positive.  Were it not -- logits that are no numbers -- lane 0 answers with an id that is neither 0 nor x)
    const int sel = hit ? __ffsll((long long)hit) - 1 : nz ? 63 - __clzll((long long)nz) : 0;
    if (lane == sel) {
        a.out[q.out] = nz ? (unsigned)i : (q.x == 1u ? 2u : 1u);
        if (a.acc) a.acc[q.out] = 0;
    }
}

} // namespace rwkvk
