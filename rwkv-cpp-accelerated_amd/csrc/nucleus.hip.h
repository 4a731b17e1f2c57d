// nucleus.hip.h -- temperature / top-p / top-k sampling with presence and frequency penalties over the 50277 logits ON THE DEVICE
// (gfx950): what the front ends of RWKV-4 models sample with, in the shape of the typical sampler (sampler.hip.h), with which it shares
// the draw record (DrawArgs: row, uniform, pick, scratch) and the helpers on it (ts_row, ts_combine, ts_pad, ts_uniform, ts_emit) as well
// as the block scan.  No reference counterpart (the reference ships typical() only).  include/rwkv_mi355x.h rwkv_sample_nucleus has the
// semantics; include/rwkv_sampler.h nucleus_u is the same draw on the host.  For one logits row l and the f32 occurrence counts c of one state slot:
//     l'_i = l_i - (presence + c_i frequency) where c_i > 0, l_i otherwise (f64); with the ban l'_0 = -99 afterwards
//     p = softmax(l');  kept = { p_i >= the p where the descending running mass reaches top_p }  and  { p_i >= the top_k-th largest p }
//     weight exp((l'_i - max l') / temp) on the kept set;  inverse CDF in token order;  c <- f32(c decay), c_pick += 1
// Neither cut needs a sort.  The key is the f32 pattern of -log p_i (>= 0, so the patterns order as the values; ascending key = descending
// p) and both thresholds are patterns found by ONE most-significant-digit-first radix select of 12 + 12 + 8 bits over two histograms in LDS:
//     top-p  thr_p = min { v : sum_{key <= v} p >= top_p }       over probability MASS (f64 bins, tokens below 1e-30 carry none: skipped)
//     top-k  thr_k = min { v : #{ key <= v } >= top_k }          over exact integer COUNTS of the 50277 real tokens (the padding is not counted)
// Each pass reads key and p once and feeds both histograms, each under its own prefix; wave 0 scans the masses while wave 1 scans the counts.
// kept = key <= min(thr_p, thr_k): ties at either cut are kept, and the most probable token always is, so the largest weight is exactly 1
// at every temp > 0.  Three launches as there: k_nucleus_stats and k_nucleus_keys (64 workgroups: the penalty is applied where the logits
// are read), k_nucleus (one workgroup of 1024 threads per row: select, draw, count update); blockIdx.y = row, each with its own scratch
// slice, pick and count vector (row r of a launch uses the counts of slot `slot` + r).
#pragma once
#include "sampler.hip.h"

namespace rwkvk {

constexpr int NU_GROUP = 10;               // tokens of a thread whose loads are issued together in k_nucleus
static_assert(TS_PER % NU_GROUP == 0, "a thread's tokens are whole groups");
constexpr int NU_LDS_BYTES = TS_NT * 8 + TS_HIST * 8 + TS_HIST * 4;      // scan, mass bins, count bins of k_nucleus (56 KiB)
static_assert(NU_LDS_BYTES + 64 <= 64 * 1024, "k_nucleus keeps its two histograms in static LDS");

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

// (2) probabilities, keys and weights, written in the selection kernel's thread-contiguous order
__global__ __launch_bounds__(TS_GT) void k_nucleus_keys(NucleusArgs a)
{
    const int V = (int)VOCAB;
    const int i0 = block_lo(V), i1 = block_hi(V);
    const float *lg = ts_row(a);
    const float *cnt = a.penalty ? nu_counts(a) : nullptr;
    double M, logZ, H;
    ts_combine(a, M, logZ, H);      // M = max l', Z = sum exp(l' - M) >= 1; H is not used (the partials carry 0 in the third word)
    for (int i = i0 + threadIdx.x; i < i1; i += TS_GT) {
        const double d = nu_logit(a, lg, cnt, i) - M;                       // <= 0, and 0 for the largest logit
        const double nl = logZ - d;                                         // -log p_i >= 0
        const size_t pos = ts_off((i % TS_PER) * TS_NT + i / TS_PER);
        a.p[pos] = (float)exp(-nl);
        a.pw[pos] = (float)exp(d * a.inv_temp);                             // exactly 1 for the largest logit
        a.key[pos] = __float_as_uint((float)nl);
    }
    if (blockIdx.x == 0) ts_pad(a);       // k_nucleus does not count the padding positions
}

// (3) both thresholds by one radix select, the draw, the count update.  Thread t owns tokens [50 t, 50 t + 50), its k-th at position
// k * TS_NT + t (k_typical's layout: every pass is coalesced).
__global__ __launch_bounds__(TS_NT) void k_nucleus(NucleusArgs a)
{
    __shared__ double scan[TS_NT];
    __shared__ double hist[TS_HIST];
    __shared__ unsigned cnth[TS_HIST];
    __shared__ int selp_bin, selk_bin;
    __shared__ double selp_before;
    __shared__ unsigned selk_before;
    __shared__ unsigned pick_s, last_s;
    const int t = threadIdx.x, i0 = t * TS_PER;
    const unsigned *key = a.key + blockIdx.y * TS_ROW;
    const float *p = a.p + blockIdx.y * TS_ROW;
    const float *pw = a.pw + blockIdx.y * TS_ROW;
    const int nreal = min(max((int)VOCAB - i0, 0), TS_PER);      // this thread's tokens below V (the rest is padding)

    const double top_p = fmax((double)a.top_p, 1e-300);          // top_p <= 0 keeps the smallest key (the most probable token and its ties)
    const unsigned top_k = a.top_k;
    unsigned prefp = 0u, prefk = 0u;
    double accp = 0.0;                   // mass of all keys below the current prefix range
    unsigned acck = 0u;                  // tokens there
    bool p_open = false;                 // the mass never reaches top_p: everything is kept
#pragma unroll 1
    for (int pass = 0; pass < 3; pass++) {
        const int shift = pass == 0 ? 20 : pass == 1 ? 8 : 0, bits = pass == 2 ? 8 : 12, nb = 1 << bits;
        for (int b = t; b < TS_HIST; b += TS_NT) { hist[b] = 0.0; cnth[b] = 0u; }
        __syncthreads();
        // in groups of NU_GROUP tokens: all loads of a group are issued (2 NU_GROUP in flight per thread) before its first LDS add.  Written as
        // one loop -- load key, load p, add -- the compiler waits for each load in front of the add behind it: two L2 round trips per token.
#pragma unroll 1
        for (int k0 = 0; k0 < TS_PER; k0 += NU_GROUP) {
            unsigned kbs[NU_GROUP];
            float pks[NU_GROUP];
#pragma unroll
            for (int j = 0; j < NU_GROUP; j++) { kbs[j] = key[(k0 + j) * TS_NT + t]; pks[j] = p[(k0 + j) * TS_NT + t]; }
#pragma unroll
            for (int j = 0; j < NU_GROUP; j++) {
                const unsigned kb = kbs[j];
                const float pk = pks[j];
                const unsigned bin = (kb >> shift) & (unsigned)(nb - 1);             // < nb <= TS_HIST
                const bool inp = pass == 0 || (kb >> (shift + bits)) == (prefp >> (shift + bits));
                if (!p_open && inp && pk > 1e-30f) __hip_atomic_fetch_add(&hist[bin], (double)pk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                const bool ink = pass == 0 || (kb >> (shift + bits)) == (prefk >> (shift + bits));
                if (top_k && ink && k0 + j < nreal) __hip_atomic_fetch_add(&cnth[bin], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        __syncthreads();
        const int per = nb / 64;
        if (t < 64 && !p_open) {
            // wave 0: lane l owns bins [l * per, (l + 1) * per); the first bin where the running mass reaches top_p
            double loc = 0.0;
            for (int b = 0; b < per; b++) loc += hist[t * per + b];
            double incl = loc;
            for (int off = 1; off < 64; off <<= 1) {
                const double v = __shfl_up(incl, off, 64);
                if (t >= off) incl += v;
            }
            double run = accp + (incl - loc);
            int found = 0x7fffffff, lastnz = -1;
            double bef = 0.0, lastbef = 0.0;
            for (int b = 0; b < per; b++) {
                const double h = hist[t * per + b];
                if (found == 0x7fffffff && h > 0.0 && run + h >= top_p) { found = t * per + b; bef = run; }
                if (h > 0.0) { lastnz = t * per + b; lastbef = run; }
                run += h;
            }
            int best = found;
            for (int off = 32; off >= 1; off >>= 1) best = min(best, __shfl_xor(best, off, 64));
            if (found == best && best != 0x7fffffff) { selp_bin = best; selp_before = bef; }
            if (best == 0x7fffffff) {
                // (wave-uniform) pass 0: the mass never reaches top_p, everything is kept.  Later passes add up the masses of the bin the pass
                // before chose in another order, and may end one rounding short of what that pass saw: the last non-empty bin then
                int far = pass > 0 ? lastnz : -1;
                for (int off = 32; off >= 1; off >>= 1) far = max(far, __shfl_xor(far, off, 64));
                if (far >= 0 && lastnz == far) { selp_bin = far; selp_before = lastbef; }
                if (t == 0 && far < 0) selp_bin = -1;
            }
        } else if (t >= 64 && t < 128 && top_k) {
            // wave 1: the same over the counts; the first bin where the running count reaches top_k (there is one: top_k < V tokens are counted)
            const int l = t - 64;
            unsigned loc = 0u;
            for (int b = 0; b < per; b++) loc += cnth[l * per + b];
            unsigned incl = loc;
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned v = __shfl_up(incl, off, 64);
                if (l >= off) incl += v;
            }
            unsigned run = acck + (incl - loc);
            int found = 0x7fffffff;
            unsigned bef = 0u;
            for (int b = 0; b < per; b++) {
                const unsigned h = cnth[l * per + b];
                if (found == 0x7fffffff && h > 0u && run + h >= top_k) { found = l * per + b; bef = run; }
                run += h;
            }
            int best = found;
            for (int off = 32; off >= 1; off >>= 1) best = min(best, __shfl_xor(best, off, 64));
            if (found == best && best != 0x7fffffff) { selk_bin = best; selk_before = bef; }
            if (l == 0 && best == 0x7fffffff) selk_bin = -1;
        }
        __syncthreads();
        if (!p_open) {
            if (selp_bin < 0) p_open = true;
            else { prefp |= (unsigned)selp_bin << shift; accp = selp_before; }
        }
        if (top_k) {
            if (selk_bin < 0) prefk = 0x7f800000u;     // (not reached with top_k < V; keys that are no numbers sort behind +inf and may leave it short)
            else { prefk |= (unsigned)selk_bin << shift; acck = selk_before; }
        }
        __syncthreads();
    }
    unsigned thr = p_open ? 0x7f800000u : prefp;
    if (top_k) thr = min(thr, prefk);

    // weights of the kept set and the inverse-CDF draw in token order (k_typical's, without its rescue: the largest weight is 1)
    double wsum = 0.0;
    // (key and weight are both loaded, then selected: `key <= thr ? pw : 0` as written is a load, a wait, a branch, a load and a wait per token)
#pragma unroll 1
    for (int k0 = 0; k0 < TS_PER; k0 += NU_GROUP) {
        unsigned kbs[NU_GROUP];
        float ws[NU_GROUP];
#pragma unroll
        for (int j = 0; j < NU_GROUP; j++) { kbs[j] = key[(k0 + j) * TS_NT + t]; ws[j] = pw[(k0 + j) * TS_NT + t]; }
#pragma unroll
        for (int j = 0; j < NU_GROUP; j++) wsum += kbs[j] <= thr ? (double)ws[j] : 0.0;
    }
    ts_block_scan(wsum, scan);
    const double total = scan[TS_NT - 1], before = scan[t] - wsum;
    const double target = ts_uniform(a) * total;
    if (t == 0) { pick_s = 0xffffffffu; last_s = 0u; }
    __syncthreads();
    if (wsum > 0.0 && target >= before && target < before + wsum) {       // the owner of the target
        double c = before;
        int sel = -1, lastkept = -1;
#pragma unroll 1
        for (int k0 = 0; k0 < TS_PER; k0 += NU_GROUP) {
            unsigned kbs[NU_GROUP];
            float ws[NU_GROUP];
#pragma unroll
            for (int j = 0; j < NU_GROUP; j++) { kbs[j] = key[(k0 + j) * TS_NT + t]; ws[j] = pw[(k0 + j) * TS_NT + t]; }
#pragma unroll
            for (int j = 0; j < NU_GROUP; j++) {
                const float w = kbs[j] <= thr ? ws[j] : 0.f;
                if (w > 0.f) { c += (double)w; lastkept = i0 + k0 + j; if (sel < 0 && target < c) sel = i0 + k0 + j; }
            }
        }
        if (sel < 0) sel = lastkept;               // rounding at the upper edge of this thread's range
        atomicMin(&pick_s, (unsigned)sel);
    }
    __syncthreads();
    if (pick_s == 0xffffffffu && total > 0.0) {
        // (block-uniform branch) the target fell into the gap of one rounding between two neighbouring threads' ranges: the last kept token
        int lastkept = -1;
        for (int k = 0; k < TS_PER; k++) if (key[k * TS_NT + t] <= thr && pw[k * TS_NT + t] > 0.f) lastkept = i0 + k;
        if (lastkept >= 0) atomicMax(&last_s, (unsigned)lastkept);
        __syncthreads();
        if (t == 0) pick_s = last_s;
        __syncthreads();
    }
    unsigned sel = pick_s;
    if (sel >= VOCAB) sel = 0;                     // nothing kept (logits that are no numbers); the padding carries no weight, so never an id >= V otherwise
    if (a.penalty && a.update) {
        // the stream's occurrence counts, in token order: f32(c decay) for every token, then + 1 for the pick -- two roundings, as the host restates it
        float *cnt = nu_counts(a);
        if (a.decay != 1.0f) {
            for (int i = t; i < (int)VOCAB; i += TS_NT) {
                float c = __fmul_rn(cnt[i], a.decay);
                if (i == (int)sel) c = __fadd_rn(c, 1.0f);
                cnt[i] = c;
            }
        } else if (t == 0) cnt[sel] = __fadd_rn(cnt[sel], 1.0f);
    }
    if (t == 0) ts_emit(a, sel);
}

} // namespace rwkvk
