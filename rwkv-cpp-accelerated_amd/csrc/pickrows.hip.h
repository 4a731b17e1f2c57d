// pickrows.hip.h -- n INDEPENDENT picks over any (logits row, count vector) pairs in one launch sequence (gfx950, wave64): the sampler of a
// continuous-batching server's step, and the pick of the sampled speculative verify.  include/rwkv_mi355x.h rwkv_sample_rows and
// rwkv_spec_sample_segments have the contracts.  No reference counterpart (the reference samples one row on the host).
//
// The samplers of sampler.hip.h / nucleus.hip.h take ONE argument record by value: blockIdx.y = r is logits row `row` + r with the counts of slot
// `slot` + r, and one temperature, top-p, top-k, penalty and step serve every row.  Here blockIdx.y = j is QUERY j of a device table (PickQ): its own
// row, its own count vector, its own parameters, its own uniform or (seed, step), its own place for the id.  A workgroup loads its query's record
// first -- the address is uniform over the workgroup, so the record arrives in scalar registers -- forms from it the NucleusArgs that the launch
// of one query alone would have carried, and runs the sampler's shared bodies on it (nu_logit, ts_combine, ts_keys, ts_select<true>, ts_kept_sum,
// ts_draw), which index the per-row scratch (part, p, key, pw) by blockIdx.y -- the query: nothing to adapt.  sampler.hip.h and nucleus.hip.h are
// untouched, so k_nucleus_* compile as before; what those three KERNELS hold themselves and no helper does -- the stats walk, the two key formulas,
// the count update -- stands here a second time, line for line, and tests/test_pick_rows_gpu.py holds every pick and every updated count vector to
// rwkv_sample_nucleus bit for bit.
//     k_pickq_stats   grid (TS_G, batch) x 256: slice p of query j's row under the query's penalty -> the (max, sum exp) partial; a GREEDY query
//                     leaves the slice's (largest logit, lowest id) with id 0 skipped in the same two words
//     k_pickq_keys    same grid: ts_keys with the query's 1 / temp; the workgroups of a greedy query return at once
//     k_pickq         grid (1, batch) x 1024: select with the query's top_p / top_k, draw with the query's u, count update of the query's slot;
//                     greedy: one wave folds the 64 slice partials by k_argmax_rows' order (larger logit, then lower id; no winner: id 0)
// Either kind writes its id to out[q.out]: the verify addresses picks by logits row, rwkv_sample_rows by query.
// A greedy query rides in the sampler's grid, not in k_argmax_rows' 16 float4 slices: rows of a table start anywhere, a mixed batch stays three
// launches, and the 64 x 786 scalar loads of a row are coalesced.  The order (am_better) is total on numbers, so the slicing does not show.
// The kinds branch on the record, per workgroup: every __syncthreads below sits under a condition that is uniform over its workgroup.
// Plain C++ and vector memory operations only; the kernels write the scratch, `out` and -- an updating query -- its own count vector.
#pragma once
#include "nucleus.hip.h"

namespace rwkvk {

// New kernels are built without gfx950's packed f32 arithmetic (v_pk_mul_f32, v_pk_fma_f32), which this project no longer takes on trust in new
// code.  The one file-wide build has no switch for it that would leave the existing kernels' code alone, so the kernels carry the attribute.  It
// touches one place: the count update's loop, where the compiler pairs two tokens; per token the operations and roundings are the same.
#define PQ_KERNEL __global__ __attribute__((target("no-packed-fp32-ops")))
constexpr unsigned PQ_NUCLEUS = 1u, PQ_PENALTY = 2u, PQ_UPDATE = 4u, PQ_BAN0 = 8u, PQ_SEED = 16u;
// One query, as the host derives it from a rwkv_pick (engine.hip make_pickq: the rules of make_sampler, derived once for both)
struct PickQ {
    unsigned row, slot;           // logits row; count vector (read with PQ_PENALTY, written with PQ_UPDATE too)
    unsigned out;                 // where the id goes: out[q.out]
    unsigned flags;               // PQ_*; without PQ_NUCLEUS the query is greedy and nothing below is read
    double inv_temp;              // 1 / temp (exactly 1 for temp == 1)
    double u;                     // uniform in [0, 1) without PQ_SEED
    unsigned long long seed, step;   // PQ_SEED: u = uniform(splitmix64(seed + step)), the draw of the decode loops at that step
    float top_p;
    unsigned top_k;               // 0: off
    float presence, frequency, decay;
    unsigned pad;
};
static_assert(sizeof(PickQ) == 72, "the query record is 72 bytes on both sides of the upload");

// What the three launches of a batch share: the table from the batch's first query on, the context's arrays, the scratch of `batch` rows
struct PickQArgs {
    const PickQ *q;               // [batch]
    const float *logits;          // [max_ctx][V]
    float *counts;                // [max_ctx][V] (nullptr when no query of the call has a penalty)
    unsigned long long *out;
    double *part;                 // [batch][TS_G][3]
    float *p;                     // [batch][TS_ROW]
    unsigned *key;
    float *pw;
};

__device__ __forceinline__ const float *pq_row(const PickQArgs &g, const PickQ &q) { return g.logits + (size_t)q.row * VOCAB; }
__device__ __forceinline__ float *pq_counts(const PickQArgs &g, const PickQ &q) { return g.counts + (size_t)q.slot * VOCAB; }      // (asked for only with PQ_PENALTY)
// the record of k_nucleus_* for this query alone.  row, slot and counts stay empty: the bodies get the row and the vector handed in.  The step
// goes into the seed (seed + step is one 64-bit sum in ts_uniform either way; DrawArgs' step is an int, a server's step count need not fit)
__device__ __forceinline__ NucleusArgs pq_nucleus(const PickQArgs &g, const PickQ &q)
{
    NucleusArgs a{};
    a.logits = g.logits;
    a.ban0 = (q.flags & PQ_BAN0) ? 1 : 0;
    a.u = q.u; a.use_seed = (q.flags & PQ_SEED) ? 1 : 0; a.seed = q.seed + q.step; a.step = 0;
    a.part = g.part; a.p = g.p; a.key = g.key; a.pw = g.pw;
    a.inv_temp = q.inv_temp; a.top_p = q.top_p; a.top_k = q.top_k;
    a.presence = q.presence; a.frequency = q.frequency; a.decay = q.decay;
    a.penalty = (q.flags & PQ_PENALTY) ? 1 : 0; a.update = (q.flags & PQ_UPDATE) ? 1 : 0;
    return a;
}

// (greedy) this workgroup's slice of the row: the largest logit and its lowest id, id 0 skipped, into words 0 and 1 of the slice's partial -- an
// f32 and a u32, both exact in an f64
__device__ __forceinline__ void pq_argmax_slice(const PickQArgs &g, const float *lg)
{
    __shared__ float sv[TS_GT / 64];
    __shared__ unsigned si[TS_GT / 64];
    const int V = (int)VOCAB;
    const int i0 = block_lo(V), i1 = block_hi(V);
    float best = -INFINITY;
    unsigned besti = 0xffffffffu;
    for (int i = i0 + threadIdx.x; i < i1; i += TS_GT) {
        const float v = lg[i];
        if (i != 0 && am_better(v, (unsigned)i, best, besti)) { best = v; besti = (unsigned)i; }
    }
    am_wave_fold(best, besti);
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = best; si[threadIdx.x >> 6] = besti; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < TS_GT / 64; w++)
            if (am_better(sv[w], si[w], best, besti)) { best = sv[w]; besti = si[w]; }
        double *part = g.part + blockIdx.y * TS_PART_ROW + blockIdx.x * 3;
        part[0] = (double)best; part[1] = (double)besti;
    }
}

// (1) a nucleus query: k_nucleus_stats' walk -- the f64 maximum of the slice, then the sum of exp(l' - max), folded in the same order (lanes, then
// the four waves in turn) -- on the query's row under the query's counts, written here because that kernel's body is not a helper
PQ_KERNEL __launch_bounds__(TS_GT) void k_pickq_stats(const PickQArgs g)
{
    __shared__ double red[RED_BYTES / 8];
    const PickQ q = g.q[blockIdx.y];
    const float *lg = pq_row(g, q);
    if (!(q.flags & PQ_NUCLEUS)) { pq_argmax_slice(g, lg); return; }
    const NucleusArgs a = pq_nucleus(g, q);
    const float *cnt = pq_counts(g, q);
    const int V = (int)VOCAB;
    const int i0 = block_lo(V), i1 = block_hi(V);
    double mx = -INFINITY;
    for (int i = i0 + threadIdx.x; i < i1; i += TS_GT) mx = fmax(mx, nu_logit(a, lg, cnt, i));
    for (int off = 32; off >= 1; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = red[0];
    for (int k = 1; k < TS_GT / 64; k++) mx = fmax(mx, red[k]);
    __syncthreads();
    double z = 0.0;
    for (int i = i0 + threadIdx.x; i < i1; i += TS_GT) { const double l = nu_logit(a, lg, cnt, i); z += l > -INFINITY ? exp(l - mx) : 0.0; }      // (a -inf logit carries no mass)
    z = wave_sum(z);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = z;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tz = 0.0;
        for (int k = 0; k < TS_GT / 64; k++) tz += red[k];
        double *part = ts_part(a) + blockIdx.x * 3;
        part[0] = mx; part[1] = tz; part[2] = 0.0;
    }
}

// (2) ts_keys with the nucleus key and weight (k_nucleus_keys' two formulas) for the query's 1 / temp
PQ_KERNEL __launch_bounds__(TS_GT) void k_pickq_keys(const PickQArgs g)
{
    const PickQ q = g.q[blockIdx.y];
    if (!(q.flags & PQ_NUCLEUS)) return;
    const NucleusArgs a = pq_nucleus(g, q);
    const float *lg = pq_row(g, q), *cnt = pq_counts(g, q);
    ts_keys(a, [&](int i) { return nu_logit(a, lg, cnt, i); }, [&](double d, double nl, double, float &pw, unsigned &key) {
        pw = (float)exp(d * a.inv_temp);
        key = __float_as_uint((float)nl);
    });
}

// (3) greedy: one wave folds the slice partials.  Nucleus: k_nucleus' sequence -- both thresholds by one select, kept sum, draw -- then the
// count update of the query's vector: f32(c decay) for every token, then + 1 for the pick, as nu_count_update
static_assert(TS_G == 64, "k_pickq folds a greedy query's slice partials with one lane each");
PQ_KERNEL __launch_bounds__(TS_NT) void k_pickq(const PickQArgs g)
{
    __shared__ double scan[TS_NT];
    const PickQ q = g.q[blockIdx.y];
    if (!(q.flags & PQ_NUCLEUS)) {
        if (threadIdx.x < 64) {
            const double *part = g.part + blockIdx.y * TS_PART_ROW + threadIdx.x * 3;
            float best = (float)part[0];
            unsigned besti = (unsigned)part[1];
            am_wave_fold(best, besti);
            if (threadIdx.x == 0) g.out[q.out] = besti < VOCAB ? besti : 0u;      // (no winner -- every logit NaN -- gives id 0, as k_argmax_rows_finish)
        }
        return;
    }
    const NucleusArgs a = pq_nucleus(g, q);
    const unsigned *key = a.key + blockIdx.y * TS_ROW;
    const float *p = a.p + blockIdx.y * TS_ROW, *pw = a.pw + blockIdx.y * TS_ROW;
    const TsCut cut = ts_select<true>(key, p, false, fmax((double)a.top_p, 1e-300), a.top_k);
    const unsigned thr = min(cut.mass, cut.count);
    const double wsum = ts_kept_sum(key, pw, thr, scan);
    const unsigned sel = ts_draw(a, key, pw, thr, wsum, scan);
    if (q.flags & PQ_UPDATE) {
        float *cnt = pq_counts(g, q);
        if (q.decay != 1.0f) {
            for (int i = threadIdx.x; i < (int)VOCAB; i += TS_NT) {
                float c = __fmul_rn(cnt[i], q.decay);
                if (i == (int)sel) c = __fadd_rn(c, 1.0f);
                cnt[i] = c;
            }
        } else if (threadIdx.x == 0) cnt[sel] = __fadd_rn(cnt[sel], 1.0f);
    }
    if (threadIdx.x == 0) g.out[q.out] = sel;
}

} // namespace rwkvk
