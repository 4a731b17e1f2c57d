// nucleus.hip.h -- temperature / top-p / top-k sampling with presence and frequency penalties over the 50277 logits ON THE DEVICE
// (gfx950): what the front ends of RWKV-4 models sample with, in the shape of the typical sampler (sampler.hip.h), whose draw record
// (DrawArgs: row, uniform, pick, scratch) with the helpers on it, keys body (ts_keys), select (ts_select) and draw (ts_kept_sum, ts_draw) it
// uses: this file holds the penalised logit, the key and weight formula, and the count update.  No reference counterpart (the reference ships
// typical() only).  include/rwkv_mi355x.h rwkv_sample_nucleus has the
// semantics; include/rwkv_sampler.h nucleus_u is the same draw on the host.  For one logits row l and the f32 occurrence counts c of one state slot:
//     l'_i = l_i - (presence + c_i frequency) where c_i > 0, l_i otherwise (f64); with the ban l'_0 = -99 afterwards
//     p = softmax(l');  kept = { p_i >= the p where the descending running mass reaches top_p }  and  { p_i >= the top_k-th largest p }
//     weight exp((l'_i - max l') / temp) on the kept set;  inverse CDF in token order;  c <- f32(c decay), c_pick += 1
// Neither cut needs a sort.  The key is the f32 pattern of -log p_i (>= 0, so the patterns order as the values; ascending key = descending
// p) and both thresholds are patterns found by one run of ts_select, over the mass histogram for top-p and the count histogram for top-k.
// kept = key <= min(thr_p, thr_k): ties at either cut are kept, and the most probable token always is, so the largest weight is exactly 1
// at every temp > 0.  Three launches as there: k_nucleus_stats and k_nucleus_keys (64 workgroups: the penalty is applied where the logits
// are read), k_nucleus (one workgroup of 1024 threads per row: select, draw, count update); blockIdx.y = row, each with its own scratch
// slice, pick and count vector (row r of a launch uses the counts of slot `slot` + r).
#pragma once
#include "sampler.hip.h"

namespace rwkvk {

struct NucleusArgs : DrawArgs {
    unsigned slot;                // count vector of blockIdx.y = 0
    double inv_temp;              // 1 / temp (exactly 1 for temp == 1)
    float top_p;
    unsigned top_k;               // 0: off (the host maps top_k >= V to 0)
    float presence, frequency, decay;
    int penalty;                  // presence != 0 || frequency != 0: `counts` is read (and, with `update`, written)
    int update;                   // after the pick: counts <- f32(counts decay), counts[pick] += 1
    float *counts;                // [max_ctx][V] occurrence counts per state slot (nullptr without penalty)
};

__device__ __forceinline__ float *nu_counts(const NucleusArgs &a) { return a.counts + (size_t)(a.slot + blockIdx.y) * VOCAB; }
// the penalised logit: every factor is an f32 widened to f64 (c frequency is exact there), the ban behind the penalty
__device__ __forceinline__ double nu_logit(const NucleusArgs &a, const float *lg, const float *cnt, int i)
{
    if (a.ban0 && i == 0) return -99.0;
    double l = (double)lg[i];
    if (a.penalty) {
        const float c = cnt[i];
        if (c > 0.f) l -= (double)a.presence + (double)c * (double)a.frequency;
    }
    return l;
}

// (1) per-workgroup online-softmax partials of the penalised row
__global__ __launch_bounds__(TS_GT) void k_nucleus_stats(NucleusArgs a)
{
    __shared__ double red[RED_BYTES / 8];
    const int V = (int)VOCAB;
    const int i0 = block_lo(V), i1 = block_hi(V);
    const float *lg = ts_row(a);
    const float *cnt = a.penalty ? nu_counts(a) : nullptr;
    double mx = -INFINITY;
    for (int i = i0 + threadIdx.x; i < i1; i += TS_GT) mx = fmax(mx, nu_logit(a, lg, cnt, i));
    for (int off = 32; off >= 1; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = red[0];
    for (int k = 1; k < TS_GT / 64; k++) mx = fmax(mx, red[k]);
    __syncthreads();
    double z = 0.0;
    // (a -inf logit carries no mass: said outright, because under a constraint a whole slice can be -inf, and -inf - mx is then no number)
    for (int i = i0 + threadIdx.x; i < i1; i += TS_GT) { const double l = nu_logit(a, lg, cnt, i); z += l > -INFINITY ? exp(l - mx) : 0.0; }
    z = wave_sum(z);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = z;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tz = 0.0;
        for (int k = 0; k < TS_GT / 64; k++) tz += red[k];
        double *part = ts_part(a);
        part[blockIdx.x * 3 + 0] = mx; part[blockIdx.x * 3 + 1] = tz; part[blockIdx.x * 3 + 2] = 0.0;
    }
}

// (2) the key is -log p_i itself; the weight is exactly 1 for the largest logit
__global__ __launch_bounds__(TS_GT) void k_nucleus_keys(NucleusArgs a)
{
    const float *lg = ts_row(a);
    const float *cnt = a.penalty ? nu_counts(a) : nullptr;
    // (ts_combine's H is not used: the partials carry 0 in the third word)
    ts_keys(a, [&](int i) { return nu_logit(a, lg, cnt, i); }, [&](double d, double nl, double, float &pw, unsigned &key) {
        pw = (float)exp(d * a.inv_temp);
        key = __float_as_uint((float)nl);
    });
}

// the stream's occurrence counts behind the pick, in token order: f32(c decay) for every token, then + 1 for the pick -- two roundings, as the host restates it
__device__ __forceinline__ void nu_count_update(const NucleusArgs &a, unsigned sel)
{
    float *cnt = nu_counts(a);
    if (a.decay != 1.0f) {
        for (int i = threadIdx.x; i < (int)VOCAB; i += TS_NT) {
            float c = __fmul_rn(cnt[i], a.decay);
            if (i == (int)sel) c = __fadd_rn(c, 1.0f);
            cnt[i] = c;
        }
    } else if (threadIdx.x == 0) cnt[sel] = __fadd_rn(cnt[sel], 1.0f);
}

// (3) both thresholds by one select, draw (k_typical's, without its rescue: the largest weight is 1), count update, emit
__global__ __launch_bounds__(TS_NT) void k_nucleus(NucleusArgs a)
{
    __shared__ double scan[TS_NT];
    const unsigned *key = a.key + blockIdx.y * TS_ROW;
    const float *p = a.p + blockIdx.y * TS_ROW;
    const float *pw = a.pw + blockIdx.y * TS_ROW;
    // top_p <= 0 keeps the smallest key (the most probable token and its ties)
    const TsCut cut = ts_select<true>(key, p, false, fmax((double)a.top_p, 1e-300), a.top_k);
    const unsigned thr = min(cut.mass, cut.count);
    const double wsum = ts_kept_sum(key, pw, thr, scan);
    const unsigned sel = ts_draw(a, key, pw, thr, wsum, scan);
    if (a.penalty && a.update) nu_count_update(a, sel);
    if (threadIdx.x == 0) ts_emit(a, sel);
}

} // namespace rwkvk
