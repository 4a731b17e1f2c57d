// floor.hip.h -- min-p and Mirostat v2 sampling over the 50277 logits ON THE DEVICE (gfx950, wave64): the two probability-FLOOR cuts.  No
// reference counterpart (the reference ships typical() only).  include/rwkv_mi355x.h rwkv_sample_floor has the semantics; include/rwkv_sampler.h
// minp_u / mirostat_u are the same draws on the host.  For one logits row l, the f32 occurrence counts c of one state slot and -- Mirostat --
// the slot's running threshold mu (f64):
//     l'_i = nu_logit (nucleus.hip.h: the penalty, the ban of id 0, -inf of a constrained row), mx = max l'
//     MINP      kept = { l'_i - mx >= lnf },  lnf = log(min_p) from the host
//     MIROSTAT  d_i = (l'_i - mx) inv_temp, Z = sum exp(d_i), S_i = (log Z - d_i) / ln 2;  kept = { S_i <= mu }, or { l'_i == mx } when that is empty
//     weight exp((l'_i - mx) inv_temp) on the kept set, inverse CDF in token order;  counts as nu_count_update;  mu <- mu - eta (S_pick - tau)
// The kept set is known per token as soon as the row's maximum (and log Z) is: no order statistic, so none of the nucleus sampler's keys,
// histograms, radix select or its 1.84 MB of key / p / weight scratch per row.  Two launches, blockIdx.y = row:
//     k_floor_stats   grid (TS_G, rows) x 256, the slice grid of k_nucleus_stats: per slice the f64 maximum of l' and -- Mirostat -- the sum of
//                     exp((l' - slice max) inv_temp), 16 bytes into the row's `part` words
//     k_floor         grid (1, rows) x 1024: every wave folds the 64 partials the same way (lanes by a fixed tree on the DPP network: no arrival order), then ONE
//                     float4-wide pass over the row: thread t owns the float4s [14 t, 14 t + 14) behind the row's first 16-byte boundary (row r starts
//                     4 r bytes past one, as in k_argmax_rows: thread 0 takes the 0 .. 3 ids in front, the last thread the 0 .. 3 behind), a
//                     contiguous run of ids, and adds up its kept weight in token order; one scan in LDS finds the run that holds u W, its
//                     owner walks the run again (224 bytes, from L2) to the id; counts, mu, emit
// The row is read twice, from where the head left it, and written never.  k_floorq_* are the same bodies on a query of the device table of
// pickrows.hip.h (rwkv_sample_rows), as k_pickq_* are for the nucleus sampler.
// k_floor: 8 KB of LDS for the scan and two words for the pick; a run goes in two groups of 7 float4, so 28 registers of the row are in flight per
// thread and the kernel stays under the 128 registers that 1024 threads leave each without scratch (profiles/floor/resources.txt; all 14 at
// once spilled 39 registers).
// Plain C++ and vector memory operations only; the kernels write `part`, the pick, the slot's count vector and the slot's mu.
#pragma once
#include "pickrows.hip.h"

namespace rwkvk {

constexpr int FL_Q4 = 14;                  // float4s of a thread of k_floor: 1024 * 14 * 4 = 57344 >= 50277
constexpr int FL_GROUP = 7;                // of which so many are loaded together
static_assert(FL_Q4 % FL_GROUP == 0, "a run is whole groups");
static_assert(TS_NT * FL_Q4 * 4 >= (int)VOCAB, "the draw's tiling covers the row");
constexpr double FL_LN2 = 0.693147180559945309417232121458;
constexpr unsigned PQ_MINP = 32u, PQ_MIROSTAT = 64u;     // PickQ.flags of a floor query (without PQ_NUCLEUS); PQ_UPDATE moves counts (with PQ_PENALTY) and mu

// NucleusArgs' row, uniform, pick, penalty and count fields as they are (top_p and top_k are not read), and the floor
struct FloorArgs : NucleusArgs {
    int miro;                     // 0: MINP, 1: MIROSTAT
    int mu_update;                // MIROSTAT: mu moves behind the pick
    double lnf;                   // MINP: log(min_p)
    double tau, eta;              // MIROSTAT
    double *mu;                   // [max_ctx] per state slot, indexed as the counts (slot + blockIdx.y)
    // [rows] the length words of the call's stop test (stop.hip.h StopArgs.len: 0 until the stream stops); nullptr: none.  A stream whose word is set
    // keeps the mu of its stop.  This stands in for a parked copy of mu and rests on the launch order of a step: k_stop_step of step k runs BEHIND
    // step k's k_floor (DecodeRun::step), so the word is still 0 at the draw whose pick stops the stream and set at every later one
    const unsigned *stopped;
};

// the wave's maximum in every lane: wave_sum's steps on the DPP network with fmax (lane 63 holds the fold of all four rows; the lanes that a row
// mask leaves out read 0 and are not read)
__device__ __forceinline__ double fl_wave_max(double v)
{
    v = fmax(v, dpp_f64<0xB1, 0xf, true>(v));
    v = fmax(v, dpp_f64<0x4E, 0xf, true>(v));
    v = fmax(v, dpp_f64<0x124, 0xf, true>(v));
    v = fmax(v, dpp_f64<0x128, 0xf, true>(v));
    v = fmax(v, dpp_f64<0x142, 0xa, false>(v));
    v = fmax(v, dpp_f64<0x143, 0xc, false>(v));
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, 63), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), 63);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// (1) this workgroup's slice: max l' and, Mirostat, sum exp((l' - max) inv_temp) -- k_nucleus_stats' walk and order of folding
__device__ __forceinline__ void fl_stats(const FloorArgs &a, const float *lg, const float *cnt)
{
    __shared__ double red[RED_BYTES / 8];
    const int V = (int)VOCAB;
    const int i0 = block_lo(V), i1 = block_hi(V);
    double mx = -INFINITY;
    for (int i = i0 + threadIdx.x; i < i1; i += TS_GT) mx = fmax(mx, nu_logit(a, lg, cnt, i));
    mx = fl_wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = red[0];
    for (int k = 1; k < TS_GT / 64; k++) mx = fmax(mx, red[k]);
    __syncthreads();
    double z = 0.0;
    if (a.miro)       // (a -inf logit carries no mass, said outright: a whole slice of a constrained row can be -inf)
        for (int i = i0 + threadIdx.x; i < i1; i += TS_GT) { const double l = nu_logit(a, lg, cnt, i); z += l > -INFINITY ? exp((l - mx) * a.inv_temp) : 0.0; }
    z = wave_sum(z);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = z;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tz = 0.0;
        for (int k = 0; k < TS_GT / 64; k++) tz += red[k];
        double *part = ts_part(a) + blockIdx.x * 3;
        part[0] = mx; part[1] = tz;
    }
}

// the row's statistics from the 64 partials, the same in every wave: mx, and log sum exp((l' - mx) inv_temp) (Mirostat; MINP: not read)
__device__ __forceinline__ void fl_combine(const FloorArgs &a, double &mx, double &logZ)
{
    const int lane = threadIdx.x & 63;
    const double *part = ts_part(a);
    const double m = lane < TS_G ? part[lane * 3] : -INFINITY, z = lane < TS_G ? part[lane * 3 + 1] : 0.0;
    const double mm = fl_wave_max(m);
    mx = mm;
    logZ = a.miro ? log(wave_sum(z > 0.0 ? z * exp((m - mm) * a.inv_temp) : 0.0)) : 0.0;
}

// which tokens are kept, from l' alone
struct FlCut {
    double mx, logZ, thr, inv_temp;
    int mode;                     // 0: l' - mx >= thr (MINP); 1: S <= thr (MIROSTAT); 2: l' == mx (MIROSTAT with nothing at or under mu)
    __device__ __forceinline__ double surprise(double l) const { return (logZ - (l - mx) * inv_temp) / FL_LN2; }
    __device__ __forceinline__ bool kept(double l) const { return mode == 0 ? l - mx >= thr : mode == 1 ? surprise(l) <= thr : l == mx; }
    __device__ __forceinline__ double weight(double l) const { return kept(l) ? exp((l - mx) * inv_temp) : 0.0; }
};

// f(i, l'_i) for the ids of thread t's run, in token order.  The four logits of a float4 go through nu_logit as a row of their own that starts
// at id `base`: the counts start there too, and the ban of id 0 holds where base is 0
template <class F>
__device__ __forceinline__ void fl_run(const FloorArgs &a, const float *lg, const float *cnt, int t, F f)
{
    const int V = (int)VOCAB;
    const int head = (int)(((16 - (reinterpret_cast<uintptr_t>(lg) & 15)) & 15) >> 2);      // ids in front of the first 16-byte boundary
    const int nb = (V - head) / 4;                                                          // float4s of the body
    if (t == 0)
        for (int i = 0; i < head; i++) f(i, nu_logit(a, lg, cnt, i));
    const float4 *body = reinterpret_cast<const float4 *>(lg + head);
    const int q0 = t * FL_Q4;
#pragma unroll 1
    for (int g0 = q0; g0 < q0 + FL_Q4 && g0 < nb; g0 += FL_GROUP) {
        float4 v[FL_GROUP];
#pragma unroll
        for (int j = 0; j < FL_GROUP; j++) v[j] = g0 + j < nb ? body[g0 + j] : float4{0.f, 0.f, 0.f, 0.f};      // a group's loads in flight together
#pragma unroll
        for (int j = 0; j < FL_GROUP; j++) {
            if (g0 + j >= nb) break;
            const int base = head + 4 * (g0 + j);
            const float x[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
            NucleusArgs b = a;
            b.ban0 = a.ban0 && base == 0;
            const float *cb = a.penalty ? cnt + base : nullptr;
#pragma unroll
            for (int k = 0; k < 4; k++) f(base + k, nu_logit(b, x, cb, k));
        }
    }
    if (t == TS_NT - 1)
        for (int i = head + 4 * nb; i < V; i++) f(i, nu_logit(a, lg, cnt, i));
}

// (2) the draw of one row: floor, kept weights per run, scan, walk, counts and mu.  Every thread returns the pick (id 0 when nothing is kept: logits
// that are no numbers).  `cnt`: the slot's counts (nullptr without a penalty); `mu`: the slot's threshold (Mirostat)
__device__ __forceinline__ unsigned fl_draw(const FloorArgs &a, const float *lg, const float *cnt, double *mu)
{
    __shared__ double scan[TS_NT];
    __shared__ unsigned pick_s, last_s;
    const int t = threadIdx.x;
    FlCut cut;
    fl_combine(a, cut.mx, cut.logZ);
    cut.inv_temp = a.inv_temp;
    if (a.miro) {
        cut.thr = *mu;
        cut.mode = cut.logZ / FL_LN2 <= cut.thr ? 1 : 2;      // the top token's surprise: the smallest
    } else { cut.thr = a.lnf; cut.mode = 0; }
    double wsum = 0.0;
    int last = -1;                       // this run's last token of non-zero weight
    fl_run(a, lg, cnt, t, [&](int i, double l) { const double w = cut.weight(l); if (w > 0.0) { wsum += w; last = i; } });
    if (t == 0) { pick_s = 0xffffffffu; last_s = 0u; }
    ts_block_scan(wsum, scan);           // (its barriers order the two words too)
    // run t owns [scan[t - 1], scan[t]): the runs' ranges meet exactly, so a target below the total has one owner
    const double total = scan[TS_NT - 1], before = t ? scan[t - 1] : 0.0;
    const double target = ts_uniform(a) * total;
    if (target >= before && target < scan[t]) {
        double c = before;
        int sel = -1;
        fl_run(a, lg, cnt, t, [&](int i, double l) { const double w = cut.weight(l); if (w > 0.0) { c += w; if (sel < 0 && target < c) sel = i; } });
        atomicMin(&pick_s, (unsigned)(sel < 0 ? last : sel));              // (sel < 0: the walk's sum ends one rounding short of the scan's)
    }
    if (last >= 0) atomicMax(&last_s, (unsigned)last);
    __syncthreads();
    // no owner although tokens are kept: u W rounded up onto the total: the last kept token (ts_draw's rule, and what the host twins return when
    // their running sum ends short of the target)
    unsigned sel = pick_s != 0xffffffffu ? pick_s : total > 0.0 ? last_s : 0u;
    if (sel >= VOCAB) sel = 0u;
    double lsel = 0.0;
    if (t == 0 && a.miro && a.mu_update) lsel = nu_logit(a, lg, cnt, (int)sel);      // under the counts in front of the update
    __syncthreads();
    if (a.penalty && a.update) nu_count_update(a, sel);
    if (t == 0 && a.miro && a.mu_update && !(a.stopped && a.stopped[blockIdx.y]))
        *mu = cut.thr - a.eta * (cut.surprise(lsel) - a.tau);
    return sel;
}

PQ_KERNEL __launch_bounds__(TS_GT) void k_floor_stats(const FloorArgs a)
{
    fl_stats(a, ts_row(a), a.penalty ? nu_counts(a) : nullptr);
}

PQ_KERNEL __launch_bounds__(TS_NT) void k_floor(const FloorArgs a)
{
    const unsigned sel = fl_draw(a, ts_row(a), a.penalty ? nu_counts(a) : nullptr, a.miro ? a.mu + (a.slot + blockIdx.y) : nullptr);
    if (threadIdx.x == 0) ts_emit(a, sel);
}

// (loops) the slots' mu at the start of a call
__global__ __launch_bounds__(64) void k_floor_mu_fill(double *mu, unsigned n, double v)
{
    const unsigned i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) mu[i] = v;
}

// ---- the same on a query of the device table (rwkv_sample_rows).  A floor query is a PickQ in size and in every shared field, so it rides in the
// one uploaded table behind the greedy and nucleus queries; where those carry top_p and top_k it carries its floor, under its own types ----
struct FloorQ {
    unsigned row, slot, out, flags;      // as PickQ; flags: PQ_MINP or PQ_MIROSTAT, PQ_PENALTY, PQ_UPDATE (counts and mu), PQ_BAN0, PQ_SEED
    double inv_temp, u;
    unsigned long long seed, step;
    union { double lnf; struct { float tau, eta; } m; };     // MINP | MIROSTAT
    float presence, frequency, decay;
    unsigned pad;
};
static_assert(sizeof(FloorQ) == sizeof(PickQ) && offsetof(FloorQ, flags) == offsetof(PickQ, flags) && offsetof(FloorQ, lnf) == offsetof(PickQ, top_p) &&
              offsetof(FloorQ, presence) == offsetof(PickQ, presence), "a floor query takes a PickQ's place in the table");
struct FloorQArgs {
    const FloorQ *q;              // [batch], floor queries only
    const float *logits;          // [max_ctx][V]
    float *counts;                // [max_ctx][V] (nullptr when no query of the call has a penalty)
    double *mu;                   // [max_ctx] (nullptr when no query is Mirostat)
    unsigned long long *out;
    double *part;                 // [batch][TS_G][3]
};

// the record of k_floor_* for this query alone.  Row, counts and mu are handed to the bodies; nu_count_update alone finds the counts itself, as
// counts + (slot + blockIdx.y) V, so `slot` is the query's less blockIdx.y (unsigned arithmetic: the sum is the query's slot again)
__device__ __forceinline__ FloorArgs fq_args(const FloorQArgs &g, const FloorQ &q)
{
    FloorArgs a{};
    a.logits = g.logits;
    a.ban0 = (q.flags & PQ_BAN0) ? 1 : 0;
    a.u = q.u; a.use_seed = (q.flags & PQ_SEED) ? 1 : 0; a.seed = q.seed + q.step; a.step = 0;
    a.part = g.part;
    a.slot = q.slot - blockIdx.y; a.counts = g.counts;
    a.inv_temp = q.inv_temp;
    a.presence = q.presence; a.frequency = q.frequency; a.decay = q.decay;
    a.penalty = (q.flags & PQ_PENALTY) ? 1 : 0; a.update = (q.flags & PQ_UPDATE) ? 1 : 0;
    a.miro = (q.flags & PQ_MIROSTAT) ? 1 : 0; a.mu_update = a.update;
    if (a.miro) { a.tau = (double)q.m.tau; a.eta = (double)q.m.eta; }
    else a.lnf = q.lnf;
    return a;
}

PQ_KERNEL __launch_bounds__(TS_GT) void k_floorq_stats(const FloorQArgs g)
{
    const FloorQ q = g.q[blockIdx.y];
    const FloorArgs a = fq_args(g, q);
    fl_stats(a, g.logits + (size_t)q.row * VOCAB, a.penalty ? g.counts + (size_t)q.slot * VOCAB : nullptr);
}

PQ_KERNEL __launch_bounds__(TS_NT) void k_floorq(const FloorQArgs g)
{
    const FloorQ q = g.q[blockIdx.y];
    const FloorArgs a = fq_args(g, q);
    const unsigned sel = fl_draw(a, g.logits + (size_t)q.row * VOCAB, a.penalty ? g.counts + (size_t)q.slot * VOCAB : nullptr, a.miro ? g.mu + q.slot : nullptr);
    if (threadIdx.x == 0) g.out[q.out] = sel;
}

} // namespace rwkvk
