// sampler.hip.h -- typical sampling over the 50277 logits ON THE DEVICE (gfx950), so that the reference's
// generation loop (examples/storygen/storygen.cpp:63-69: out[0] = -99; typical(out, temp, tau)) needs no
// 201 KB logits download and no host sort per token.
//
// Behavioural mirror of reference include/rwkv/sampler/typical.h:20-58.  Two modes (include/rwkv_sampler.h has the
// findings): recipe = 0 (default) is what the reference COMPUTES -- a draw from softmax^n, n = uint8(1/temp), its cut at
// tau being a no-op -- and needs no selection at all; recipe = 1 is the recipe its header comment documents (softmax,
// entropy H, sort by |-log p - H|, keep the smallest prefix whose cumulative probability reaches tau, p^(1/temp), draw).
// For the latter the sort is not needed: with s_i = |-log p_i - H| the cut-off value is
//     thr = min { v in {s_i} : sum_{s_i <= v} p_i >= tau }
// (the sorted prefix crosses tau exactly at the first element of that value), found as a 32-bit float
// pattern by a three-pass radix select over probability-mass histograms in LDS.  Three launches:
// k_typical_stats (64 workgroups: online-softmax partials), k_typical_keys (64 workgroups: p_i and s_i as
// f32, every sum in f64) and k_typical (one workgroup of 1024 threads: select, rescue, draw).  The select (ts_select), the draw (ts_kept_sum,
// ts_draw) and the body of the keys kernel (ts_keys) are written once here for this sampler and the nucleus one (nucleus.hip.h), which differ in
// the logit, the key and weight formula and the target of the select.  The draw is the inverse CDF in token order for a uniform
// u supplied by the caller or derived from (seed, step) with splitmix64 -- include/rwkv_sampler.h has the
// same deterministic draw on the host (typical_u), which is what the parity test compares against.
// One launch covers `rows` consecutive logits rows (blockIdx.y = row, each with its own slice of the scratch arrays
// and its own pick): the batched decode samples all of its streams with the same three launches.
#pragma once
#include "kernels.hip.h"

namespace rwkvk {

constexpr int TS_NT = 1024;                // threads of the selection kernel
constexpr int TS_PER = 50;                 // tokens per thread there: 1024 * 50 = 51200 >= 50277
constexpr int TS_HIST = 4096;              // mass-histogram bins of a radix-select pass (12 bits)
constexpr int TS_G = 64;                   // workgroups of the two element-wise kernels
constexpr int TS_GT = 256;                 // threads of those
constexpr int TS_GROUP = 10;               // tokens of a thread whose loads are issued together there (ts_load_group)
static_assert(TS_NT * TS_PER >= (int)VOCAB, "sampler tiling must cover the vocabulary");
static_assert(TS_PER % TS_GROUP == 0, "a thread's tokens are whole groups");
constexpr size_t TS_PART_ROW = (size_t)TS_G * 3;           // doubles of `part` per row
constexpr size_t TS_ROW = (size_t)TS_NT * TS_PER;          // elements of `p` / `key` / `pw` per row
constexpr double TS_RESCALE = 0x1p-60;     // a total of the relative weights below this: form them again relative to the kept maximum (k_typical)

// What every sampler's draw needs, whichever way the weights are formed: the row, the uniform, where the pick goes, the per-row scratch.
// TypicalArgs (below) and NucleusArgs (nucleus.hip.h) embed it and add what is their own.
struct DrawArgs {
    const float *logits;          // [rows][V]
    int row;                      // logits row of blockIdx.y = 0 (< 0: ctl->out_row); blockIdx.y = r samples the row r behind it
    Ctl *ctl;                     // token / step feedback (device-side generation loop)
    unsigned long long *gen;      // generated ids, gen[step] (feedback)
    unsigned gen_cap;
    int ban0;                     // logits[0] = -99 before sampling (storygen.cpp:66)
    int feedback;                 // write the pick into ctl->token and advance ctl->step
    unsigned long long *pick;     // [rows] the sampled ids (nullptr: none)
    double u;                     // uniform in [0, 1) when use_seed == 0
    unsigned long long seed;      // else u = uniform(splitmix64(seed + step))
    const unsigned long long *seeds;   // per-row seeds (device, [rows]); nullptr: `seed` for every row
    int step;                     // the step of the draw; < 0: ctl->step
    int use_seed;
    double *part;                 // [rows][TS_G][3] per-workgroup (max, sum exp(l - max), sum exp(l - max) (l - max)); nucleus: l' for l, 0 in the third word
    float *p;                     // [rows][TS_NT * TS_PER] probabilities, position (i % TS_PER) * TS_NT + i / TS_PER for token i
    unsigned *key;                // same layout: bit patterns of |-log p - H| (typical), of -log p (nucleus)
    float *pw;                    // same layout: (p / p_max)^expo, the weight of typical.h:49-52 relative to the largest one (k_typical's rescue forms them again).  Nucleus: exp((l' - M) / temp)
};

struct TypicalArgs : DrawArgs {
    float tau;
    int recipe;                   // 1: the recipe typical.h documents (cut at tau, p^(1/temp)); 0: what it computes (no cut, p^uint8(1/temp))
    double expo;                  // the exponent applied to p
};

__device__ __forceinline__ const float *ts_row(const DrawArgs &a) { return a.logits + (size_t)((a.row >= 0 ? (unsigned)a.row : a.ctl->out_row) + blockIdx.y) * VOCAB; }
// this row's slices of the scratch arrays
__device__ __forceinline__ double *ts_part(const DrawArgs &a) { return a.part + blockIdx.y * TS_PART_ROW; }
__device__ __forceinline__ size_t ts_off(int pos) { return blockIdx.y * TS_ROW + (size_t)pos; }
__device__ __forceinline__ float ts_logit(const DrawArgs &a, const float *lg, int i) { return (a.ban0 && i == 0) ? -99.0f : lg[i]; }
// the padding positions: tokens V .. TS_NT * TS_PER - 1 carry no mass, no weight and the largest key (one workgroup of TS_GT threads per row)
__device__ __forceinline__ void ts_pad(const DrawArgs &a)
{
    for (int i = (int)VOCAB + threadIdx.x; i < TS_NT * TS_PER; i += TS_GT) {
        const size_t pos = ts_off((i % TS_PER) * TS_NT + i / TS_PER);
        a.p[pos] = 0.f; a.pw[pos] = 0.f; a.key[pos] = 0x7f800000u;
    }
}
// the uniform of this row and step: the caller's, or from (seed, step) -- include/rwkv_sampler.h has the same draw on the host
__device__ __forceinline__ double ts_uniform(const DrawArgs &a)
{
    if (!a.use_seed) return a.u;
    const unsigned long long seed = a.seeds ? a.seeds[blockIdx.y] : a.seed;
    const unsigned long long step = a.step >= 0 ? (unsigned long long)a.step : (unsigned long long)a.ctl->step;
    unsigned long long x = seed + step + 0x9E3779B97F4A7C15ull;   // splitmix64
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (double)(x >> 11) * (1.0 / 9007199254740992.0);
}
// (one thread per row) the pick of this row goes out, and with `feedback` into the device-side generation loop
__device__ __forceinline__ void ts_emit(const DrawArgs &a, unsigned sel)
{
    if (a.pick) a.pick[blockIdx.y] = sel;
    if (a.feedback) {
        const unsigned st = a.ctl->step;
        if (st < a.gen_cap) a.gen[st] = sel;
        a.ctl->token = sel;
        a.ctl->step = st + 1;
    }
}

// (1) per-workgroup online-softmax partials over a slice of the vocabulary
__global__ __launch_bounds__(TS_GT) void k_typical_stats(TypicalArgs a)
{
    __shared__ double red[RED_BYTES / 8];
    const int V = (int)VOCAB;
    const int i0 = block_lo(V), i1 = block_hi(V);
    const float *lg = ts_row(a);
    float mx[1] = {-INFINITY};
    for (int i = i0 + threadIdx.x; i < i1; i += TS_GT) mx[0] = fmaxf(mx[0], ts_logit(a, lg, i));
    {   // workgroup max (TS_GT / 64 waves)
        float *rf = reinterpret_cast<float *>(red);
        const float w = wave_max(mx[0]);
        if ((threadIdx.x & 63) == 0) rf[threadIdx.x >> 6] = w;
        __syncthreads();
        float m = -INFINITY;
        for (int k = 0; k < TS_GT / 64; k++) m = fmaxf(m, rf[k]);
        mx[0] = m;
        __syncthreads();
    }
    double z = 0.0, sl = 0.0;
    for (int i = i0 + threadIdx.x; i < i1; i += TS_GT) {
        const double d = (double)ts_logit(a, lg, i) - (double)mx[0];
        const double e = exp(d);
        z += e; sl += e * d;
    }
    z = wave_sum(z); sl = wave_sum(sl);
    if ((threadIdx.x & 63) == 0) { red[(threadIdx.x >> 6) * 2] = z; red[(threadIdx.x >> 6) * 2 + 1] = sl; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tz = 0.0, ts = 0.0;
        for (int k = 0; k < TS_GT / 64; k++) { tz += red[2 * k]; ts += red[2 * k + 1]; }
        double *part = ts_part(a);
        part[blockIdx.x * 3 + 0] = (double)mx[0]; part[blockIdx.x * 3 + 1] = tz; part[blockIdx.x * 3 + 2] = ts;
    }
}

// combine the partials: M = max, Z = sum exp(l - M), H = entropy = log Z - sum p (l - M)   (typical.h:29-31)
__device__ __forceinline__ void ts_combine(const DrawArgs &a, double &M, double &logZ, double &H)
{
    const int lane = threadIdx.x & 63;
    const double *part = ts_part(a);
    const double m = lane < TS_G ? part[lane * 3] : -INFINITY, z = lane < TS_G ? part[lane * 3 + 1] : 0.0, sl = lane < TS_G ? part[lane * 3 + 2] : 0.0;
    double mm = m;
    for (int off = 32; off >= 1; off >>= 1) mm = fmax(mm, __shfl_xor(mm, off, 64));
    const double sc = lane < TS_G ? exp(m - mm) : 0.0;
    const double Z = wave_sum(sc * z), S = wave_sum(sc * (sl + (m - mm) * z));
    M = mm; logZ = log(Z); H = logZ - S / Z;
}
static_assert(TS_G <= 64, "one lane per partial");

// (2) probabilities, keys and weights of one kind, written in the selection kernel's thread-contiguous order.  logit(i) is the kind's
// logit of token i; form(d, nl, H, pw, key) writes its weight and key from d = l_i - M (<= 0, and 0 for the largest logit) and nl = -log p_i
template <class Logit, class Form>
__device__ __forceinline__ void ts_keys(const DrawArgs &a, Logit logit, Form form)
{
    const int V = (int)VOCAB;
    const int i0 = block_lo(V), i1 = block_hi(V);
    double M, logZ, H;
    ts_combine(a, M, logZ, H);
    for (int i = i0 + threadIdx.x; i < i1; i += TS_GT) {
        const double d = (double)logit(i) - M;
        const double nl = logZ - d;
        const size_t pos = ts_off((i % TS_PER) * TS_NT + i / TS_PER);
        a.p[pos] = (float)exp(-nl);
        form(d, nl, H, a.pw[pos], a.key[pos]);
    }
    if (blockIdx.x == 0) ts_pad(a);       // the select does not count the padding positions
}

__global__ __launch_bounds__(TS_GT) void k_typical_keys(TypicalArgs a)
{
    const float *lg = ts_row(a);
    const double it = a.expo;
    ts_keys(a, [&](int i) { return ts_logit(a, lg, i); }, [&](double d, double nl, double H, float &pw, unsigned &key) {
        // (p_i / p_max)^expo: the weight RELATIVE to the largest one, which is exactly 1 whatever temp is (p^expo itself is below
        // f32 for every token once p_max^expo is); p^0 = 1 even for p = 0, as nc::power.  Here: 64 workgroups share the exponentials
        pw = it == 0.0 ? 1.0f : (float)exp(d * it);
        key = __float_as_uint((float)fabs(nl - H));                         // typical.h:32
    });
}

__device__ __forceinline__ double ts_block_max(double v, double *red)
{
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    __syncthreads();              // previous users of `red` are done
    if (lane == 0) red[w] = v;
    __syncthreads();
    double m = red[0];
#pragma unroll
    for (int i = 1; i < TS_NT / 64; i++) m = fmax(m, red[i]);
    return m;
}

// inclusive scan of the per-thread values into scan[TS_NT]: Hillis-Steele in LDS
__device__ __forceinline__ void ts_block_scan(double v, double *scan)
{
    const int t = threadIdx.x;
    __syncthreads();              // previous readers of `scan` are done
    scan[t] = v;
    __syncthreads();
    for (int off = 1; off < TS_NT; off <<= 1) {
        const double a = t >= off ? scan[t - off] : 0.0;
        __syncthreads();
        scan[t] += a;
        __syncthreads();
    }
}

// ---- (3) the selection kernel's pieces: one workgroup of TS_NT threads per row.  Thread t owns tokens [50 t, 50 t + 50); its k-th token sits
// at position k * TS_NT + t, so every pass over the (L2-resident) arrays is coalesced. ----

// A thread's tokens go in groups of TS_GROUP: all loads of a group are issued (2 TS_GROUP in flight per thread) before the group's first use.
// Written as one loop -- load key, load x, add to an LDS bin or select by the key -- the compiler waits for each load in front of the use
// behind it: two L2 round trips per token.
template <class X>
__device__ __forceinline__ void ts_load_group(const unsigned *key, const X *x, int k0, unsigned (&kbs)[TS_GROUP], X (&xs)[TS_GROUP])
{
#pragma unroll
    for (int j = 0; j < TS_GROUP; j++) { kbs[j] = key[(k0 + j) * TS_NT + threadIdx.x]; xs[j] = x[(k0 + j) * TS_NT + threadIdx.x]; }
}

// (one wave; lane l owns bins [l * per, (l + 1) * per) of h) the first bin where the running total -- `acc` in front of bin 0, added up in the
// order lane-local sum, scan over the lanes, bin by bin -- reaches `target`, and the total in front of that bin.  No such bin: *bin = -1 in the
// first pass.  A later pass adds up, in another order, what the pass before saw in the bin it chose, and a mass may end one rounding short of
// what that pass saw: then the last non-empty bin and the total in front of it.
template <class T>
__device__ __forceinline__ void ts_bin_search(const T *h, int per, T acc, T target, bool later, int *bin, T *before)
{
    const int l = threadIdx.x & 63;
    T loc = 0;
    for (int b = 0; b < per; b++) loc += h[l * per + b];
    T incl = loc;                                  // inclusive scan over the 64 lanes
    for (int off = 1; off < 64; off <<= 1) {
        const T v = __shfl_up(incl, off, 64);
        if (l >= off) incl += v;
    }
    T run = acc + (incl - loc);
    int found = 0x7fffffff, lastnz = -1;
    T bef = 0, lastbef = 0;
    for (int b = 0; b < per; b++) {
        const T v = h[l * per + b];
        if (found == 0x7fffffff && v > 0 && run + v >= target) { found = l * per + b; bef = run; }
        if (v > 0) { lastnz = l * per + b; lastbef = run; }
        run += v;
    }
    int best = found;
    for (int off = 32; off >= 1; off >>= 1) best = min(best, __shfl_xor(best, off, 64));
    if (found == best && best != 0x7fffffff) { *bin = best; *before = bef; }
    if (best == 0x7fffffff) {                      // (wave-uniform)
        int far = later ? lastnz : -1;
        for (int off = 32; off >= 1; off >>= 1) far = max(far, __shfl_xor(far, off, 64));
        if (far >= 0 && lastnz == far) { *bin = far; *before = lastbef; }
        if (l == 0 && far < 0) *bin = -1;
    }
}

struct TsCut { unsigned mass, count; };            // thresholds as key bit patterns, each <= 0x7f800000 (+inf): nothing is cut
template <bool COUNTS> struct TsSelectLds { double hist[TS_HIST]; double before; int bin; };
template <> struct TsSelectLds<true> : TsSelectLds<false> { unsigned cnth[TS_HIST]; unsigned kbefore; int kbin; };
static_assert(TS_NT * 8 + sizeof(TsSelectLds<true>) + 64 <= 64 * 1024, "scan and both histograms fit the static LDS of a workgroup");

// The thresholds of one row, found as bit patterns (monotone for non-negative floats) by ONE most-significant-digit-first radix select
// over histograms in LDS, 12 + 12 + 8 bits:
//     mass   = min { v : sum_{key <= v} p >= target }       over probability MASS (f64 bins; tokens that cannot move an f64 sum, p < 1e-30, are skipped).
//              If the total never reaches the target nothing is cut (typical.h: the cutoff clamps to the last index)
//     count  = min { v : #{ key <= v } >= top_k }           (COUNTS and top_k > 0) over exact integer COUNTS of the V real tokens (the padding is not counted)
// Each pass reads key and p once and feeds both histograms, each under its own prefix; wave 0 scans the masses while wave 1 scans the counts.
// `p_open`: the mass cut is off from the start; without COUNTS no pass runs then (k_typical's default mode).
template <bool COUNTS>
__device__ __forceinline__ TsCut ts_select(const unsigned *key, const float *p, bool p_open, double target, unsigned top_k)
{
    __shared__ TsSelectLds<COUNTS> s;
    const int t = threadIdx.x;
    const int nreal = min(max((int)VOCAB - t * TS_PER, 0), TS_PER);      // this thread's tokens below V (the rest is padding)
    unsigned prefp = 0u, prefk = 0u;
    double accp = 0.0;                   // mass of all keys below the current prefix range
    unsigned acck = 0u;                  // tokens there
#pragma unroll 1
    for (int pass = 0; pass < 3 && (COUNTS || !p_open); pass++) {
        const int shift = pass == 0 ? 20 : pass == 1 ? 8 : 0, bits = pass == 2 ? 8 : 12, nb = 1 << bits;
        for (int b = t; b < TS_HIST; b += TS_NT) {
            s.hist[b] = 0.0;
            if constexpr (COUNTS) s.cnth[b] = 0u;
        }
        __syncthreads();
#pragma unroll 1
        for (int k0 = 0; k0 < TS_PER; k0 += TS_GROUP) {
            unsigned kbs[TS_GROUP];
            float pks[TS_GROUP];
            ts_load_group(key, p, k0, kbs, pks);
#pragma unroll
            for (int j = 0; j < TS_GROUP; j++) {
                const unsigned kb = kbs[j];
                const float pk = pks[j];
                const unsigned bin = (kb >> shift) & (unsigned)(nb - 1);             // < nb <= TS_HIST
                const bool inp = pass == 0 || (kb >> (shift + bits)) == (prefp >> (shift + bits));
                if (!p_open && inp && pk > 1e-30f) __hip_atomic_fetch_add(&s.hist[bin], (double)pk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if constexpr (COUNTS) {
                    const bool ink = pass == 0 || (kb >> (shift + bits)) == (prefk >> (shift + bits));
                    if (top_k && ink && k0 + j < nreal) __hip_atomic_fetch_add(&s.cnth[bin], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
        __syncthreads();
        if (t < 64 && !p_open) ts_bin_search(s.hist, nb / 64, accp, target, pass > 0, &s.bin, &s.before);
        if constexpr (COUNTS)      // (there is such a bin: top_k < V tokens are counted, exactly, so the later passes never end short)
            if (t >= 64 && t < 128 && top_k) ts_bin_search(s.cnth, nb / 64, acck, top_k, pass > 0, &s.kbin, &s.kbefore);
        __syncthreads();
        if (!p_open) {
            if (s.bin < 0) p_open = true;
            else { prefp |= (unsigned)s.bin << shift; accp = s.before; }
        }
        if constexpr (COUNTS)
            if (top_k) {
                if (s.kbin < 0) prefk = 0x7f800000u;   // (not reached with top_k < V; keys that are no numbers sort behind +inf and may leave it short)
                else { prefk |= (unsigned)s.kbin << shift; acck = s.kbefore; }
            }
        __syncthreads();
    }
    return TsCut{p_open ? 0x7f800000u : prefp, COUNTS && top_k ? prefk : 0x7f800000u};
}

// the kept weights `key <= thr ? pw : 0` of this thread's tokens: their sum (returned) and its inclusive scan over the threads (scan[TS_NT])
__device__ __forceinline__ double ts_kept_sum(const unsigned *key, const float *pw, unsigned thr, double *scan)
{
    double wsum = 0.0;
#pragma unroll 1
    for (int k0 = 0; k0 < TS_PER; k0 += TS_GROUP) {
        unsigned kbs[TS_GROUP];
        float ws[TS_GROUP];
        ts_load_group(key, pw, k0, kbs, ws);
#pragma unroll
        for (int j = 0; j < TS_GROUP; j++) wsum += kbs[j] <= thr ? (double)ws[j] : 0.0;
    }
    ts_block_scan(wsum, scan);
    return wsum;
}

// the inverse-CDF draw in token order over the kept weights, behind ts_kept_sum; every thread returns the pick (id 0 when nothing is kept)
__device__ __forceinline__ unsigned ts_draw(const DrawArgs &a, const unsigned *key, const float *pw, unsigned thr, double wsum, const double *scan)
{
    __shared__ unsigned pick_s, last_s;
    const int t = threadIdx.x, i0 = t * TS_PER;
    const double total = scan[TS_NT - 1], before = scan[t] - wsum;
    const double target = ts_uniform(a) * total;
    if (t == 0) { pick_s = 0xffffffffu; last_s = 0u; }
    __syncthreads();
    if (wsum > 0.0 && target >= before && target < before + wsum) {       // the owner of the target
        double c = before;
        int sel = -1, lastkept = -1;
#pragma unroll 1
        for (int k0 = 0; k0 < TS_PER; k0 += TS_GROUP) {
            unsigned kbs[TS_GROUP];
            float ws[TS_GROUP];
            ts_load_group(key, pw, k0, kbs, ws);
#pragma unroll
            for (int j = 0; j < TS_GROUP; j++) {
                const float w = kbs[j] <= thr ? ws[j] : 0.f;
                if (w > 0.f) { c += (double)w; lastkept = i0 + k0 + j; if (sel < 0 && target < c) sel = i0 + k0 + j; }
            }
        }
        if (sel < 0) sel = lastkept;               // rounding at the upper edge of this thread's range
        atomicMin(&pick_s, (unsigned)sel);
    }
    __syncthreads();
    if (pick_s == 0xffffffffu && total > 0.0) {
        // (block-uniform branch) no owner although tokens are kept: the ranges [before, before + wsum) of two neighbouring threads can
        // leave a gap of one rounding of the scan (~1e-16 of the total) and the target fell into one.  The last kept token, which is
        // what typical_u returns when its running sum ends short of the target.
        int lastkept = -1;
        for (int k = 0; k < TS_PER; k++) if (key[k * TS_NT + t] <= thr && pw[k * TS_NT + t] > 0.f) lastkept = i0 + k;
        if (lastkept >= 0) atomicMax(&last_s, (unsigned)lastkept);
        __syncthreads();
        if (t == 0) pick_s = last_s;
        __syncthreads();
    }
    const unsigned sel = pick_s;
    // nothing kept (total == 0 or NaN: logits that are no numbers; an underflow of the weights does not come here).  The padding carries no
    // weight, so never an id >= V otherwise
    return sel >= VOCAB ? 0u : sel;
}

// (block-uniform, k_typical in recipe mode) the kept set lies so far below the largest logit -- which the cut may well drop, being the least
// typical token -- that its weights relative to p_max leave f32: form them again relative to the largest KEPT logit, from the logits, with
// 0 for every token that is cut, and sum and scan them as ts_kept_sum does.  Never needed in default mode (everything is kept, the largest
// weight is 1) nor with expo = 0 (every weight is 1).
__device__ __forceinline__ double ts_rescue(const TypicalArgs &a, const unsigned *key, float *pw, unsigned thr, double *scan)
{
    __shared__ double red[TS_NT / 64];
    const int t = threadIdx.x, i0 = t * TS_PER;
    const float *lg = ts_row(a);
    double mx = -INFINITY;
    for (int k = 0; k < TS_PER; k++)
        if (i0 + k < (int)VOCAB && key[k * TS_NT + t] <= thr) mx = fmax(mx, (double)ts_logit(a, lg, i0 + k));
    mx = ts_block_max(mx, red);
    double wsum = 0.0;
    for (int k = 0; k < TS_PER; k++) {
        const bool kept = i0 + k < (int)VOCAB && key[k * TS_NT + t] <= thr;
        const float w = kept ? (float)exp(((double)ts_logit(a, lg, i0 + k) - mx) * a.expo) : 0.f;
        pw[k * TS_NT + t] = w;                     // own positions only
        wsum += (double)w;
    }
    ts_block_scan(wsum, scan);
    return wsum;
}

// (3) select (recipe mode only: as compiled the reference cuts nothing, typical.h:50), rescue, draw, emit
__global__ __launch_bounds__(TS_NT) void k_typical(TypicalArgs a)
{
    __shared__ double scan[TS_NT];
    const unsigned *key = a.key + blockIdx.y * TS_ROW;     // this row's slices
    const float *p = a.p + blockIdx.y * TS_ROW;
    float *pw = a.pw + blockIdx.y * TS_ROW;
    // tau <= 0 keeps the smallest key, as the reference's cutoff = 0 does
    const unsigned thr = ts_select<false>(key, p, !a.recipe, fmax((double)a.tau, 1e-300), 0u).mass;
    // GUARANTEED: the kept token of largest weight has a normal f32 weight whatever temp is -- 1 in default mode, and in recipe mode
    // either the total is at least TS_RESCALE or the weights are formed again with that token at 1 -- so the pick is a kept
    // token unless the kept set is empty.
    double wsum = ts_kept_sum(key, pw, thr, scan);
    if (scan[TS_NT - 1] < TS_RESCALE) wsum = ts_rescue(a, key, pw, thr, scan);
    const unsigned sel = ts_draw(a, key, pw, thr, wsum, scan);
    if (threadIdx.x == 0) ts_emit(a, sel);
}

} // namespace rwkvk
