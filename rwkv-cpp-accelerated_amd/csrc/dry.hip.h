// dry.hip.h -- DRY ("don't repeat yourself") and no-repeat-n-gram penalties for the device decode loops (gfx950, wave64): a penalty on the id
// that would EXTEND a repeat of the stream's own tail.  include/rwkv_mi355x.h rwkv_decode_batch_dry has the contract, include/rwkv_sampler.h
// dry_scan / dry_table are the same search and the same table on the host.  No reference counterpart (the reference only samples).
//
// No pick kernel knows about the penalty.  A DRY call is a constrained call (constrain.hip.h): the step's one launch here runs between
// k_constrain_rows and the pick, and subtracts from the stream's CONSTRAINED row; the model's logits are never written.
//     k_dry_scan<false>   grid (streams), one workgroup per stream, nothing ordered across workgroups, nothing read by the host.
//                         APPEND the id this step feeds to the slot's history -- a ring of DRY_MAX_WINDOW ids and a total length per state slot,
//                         persistent across calls like the penalty counts -- unless the stopper has ended the stream (its length word is set:
//                         the history ends at the stop, and the workgroup leaves at once).  Then SCAN and PENALISE:
//     the scan            h[0 .. n - 1] = the newest min(total, window) ids, last = h[n - 1].  n < 2 or `last` a breaker: nothing.  Every start
//                         j <= n - 2 with h[j] == last is a hit: m_j = the longest run h[j - k] == h[n - 1 - k], k = 0 .. m_j - 1, that stays
//                         inside the window, holds no breaker and is no longer than DRY_MAX_MATCH (it may overlap the tail); its follower
//                         t = h[j + 1] gets L_t = max m_j.  t is penalised when L_t >= allowed: c_t <- c_t - pen[L_t - allowed], one f32 subtraction
//     k_dry_scan<true>    the scan alone over the history as it stands (no append, no row): the penalised (id, L) pairs and their count (tests)
// HOW THE DATA MOVES.  The window is staged ONCE from the ring into LDS (16 KB at most) by dword loads that unwrap the ring -- lane i reads ring
// word (base + i) mod 4096: consecutive lanes, consecutive words, one wrap per window.  The tail's DRY_MAX_MATCH newest ids are staged beside it,
// newest first, with DRY_NONE where the id is a breaker or lies in front of the window: the backward walk of a hit is then ONE compare per id --
// a breaker on either side and the window's start end it by themselves, and the walk never reads the breaker list.  Threads take the starts
// j = tid, tid + NT, ... (consecutive lanes, consecutive LDS words: no bank conflicts); one LDS read rejects a start that is no hit.
// Hits meet in an LDS open-addressing table keyed by follower id: DRY_TABLE = 8192 entries (two u32 arrays, 64 KB), bucket id mod 8192, linear
// probing, the key claimed by an LDS compare-and-swap, the lengths merged by an LDS atomic max.  At most 4095 followers exist, so the load factor
// stays <= 0.5 and a probe always ends; a max does not depend on the order of its operands, so the result is deterministic without a sort.
// Behind a barrier the table is swept: every entry with L >= allowed does the one read-modify-write on its row element.  The ids of a table are
// distinct, and a row belongs to one workgroup: no global atomic, no [50277]-sized scratch, nothing cleared in HBM, no second launch.
// The kernel is a template, so that hipcc emits it where the host code first names it -- behind every kernel of the decode and chunk paths
// (beam.hip.h k_beam_select has the measurement).  Plain C++ and vector memory operations only.
// OUT OF SCOPE: DRY in rwkv_pick_constrained, rwkv_sample_rows, beam search and the speculative calls; breaker STRINGS of several tokens (a
// breaker is one id); windows above DRY_MAX_WINDOW.
#pragma once
#include "kernels.hip.h"

namespace rwkvk {

constexpr int DRY_NT = 256;                       // threads of the workgroup (four waves)
constexpr unsigned DRY_MAX_WINDOW = 4096u;        // RWKV_DRY_MAX_WINDOW: ids of a slot's ring (a power of two: the ring index is a mask)
constexpr unsigned DRY_MAX_MATCH = 64u;           // RWKV_DRY_MAX_MATCH: the cap of a match, and the entries of the penalty table
constexpr unsigned DRY_MAX_BREAKERS = 32u;        // RWKV_DRY_MAX_BREAKERS
constexpr unsigned DRY_TABLE = 8192u;             // entries of the LDS table: twice the followers a window can have
constexpr unsigned DRY_NONE = 0xFFFFFFFFu;        // no id: an empty table key, a tail position that ends every match
static_assert((DRY_MAX_WINDOW & (DRY_MAX_WINDOW - 1u)) == 0u && DRY_TABLE >= 2u * DRY_MAX_WINDOW && (DRY_TABLE & (DRY_TABLE - 1u)) == 0u,
              "ring and table indices are masks; the table's load factor stays <= 0.5");
static_assert(DRY_MAX_MATCH <= (unsigned)DRY_NT && DRY_TABLE % (4u * DRY_NT) == 0u, "one thread per tail position; the table is cleared in whole 16-byte stores");

// passed by value with every launch (472 bytes)
struct DryArgs {
    unsigned *ring;                        // [max_ctx][DRY_MAX_WINDOW]: id number i of a slot (counted from its first) sits at word i mod DRY_MAX_WINDOW
    unsigned long long *total;             // [max_ctx]: the ids a slot has been given, also those the ring no longer holds
    unsigned slot;                         // slot of blockIdx.x = 0; blockIdx.x = s handles the slot s behind it, its row is row s of `rows`
    const unsigned long long *fed;         // [n] the ids this step feeds: ids row k of a call of many streams, the control block's token of one
    const unsigned *stopped;               // [n] the stopper's lengths (the word k_stop_step sets): != 0, the stream has ended
    float *rows;                           // [max_ctx][V] the constrained rows (k_constrain_rows has written row s in front of this launch)
    unsigned allowed, window, n_breakers;  // 1 .. DRY_MAX_MATCH, 1 .. DRY_MAX_WINDOW, 0 .. DRY_MAX_BREAKERS
    unsigned breakers[DRY_MAX_BREAKERS];
    float pen[DRY_MAX_MATCH];              // pen[i]: what L = allowed + i costs (the host's f64 table, rounded once)
    unsigned *dbg;                         // k_dry_scan<true>: count | id [DRY_MAX_WINDOW] | L [DRY_MAX_WINDOW]
};

template <bool DEBUG> __global__ __launch_bounds__(DRY_NT) void k_dry_scan(const DryArgs a)
{
    __shared__ unsigned h[DRY_MAX_WINDOW];
    __shared__ uint4 key4[DRY_TABLE / 4], len4[DRY_TABLE / 4];
    __shared__ unsigned tail[DRY_MAX_MATCH];
    __shared__ float pen[DRY_MAX_MATCH];
    __shared__ unsigned hits, count;
    unsigned *key = reinterpret_cast<unsigned *>(key4), *len = reinterpret_cast<unsigned *>(len4);
    const unsigned s = blockIdx.x, tid = threadIdx.x;
    const size_t slot = (size_t)a.slot + s;
    unsigned *ring = a.ring + slot * DRY_MAX_WINDOW;
    unsigned long long tot = a.total[slot];
    unsigned g = DRY_NONE;
    if (DEBUG) {
        if (tid == 0) a.dbg[0] = 0u;               // (the same thread writes the count at the end)
    } else {
        if (a.stopped && a.stopped[s]) return;     // the whole workgroup: the history of a stopped stream ends at its stop
        g = (unsigned)a.fed[s];
        __syncthreads();                           // every thread has read the length in front of thread 0's store
        if (tid == 0) { ring[tot & (DRY_MAX_WINDOW - 1u)] = g; a.total[slot] = tot + 1ull; }
        tot += 1ull;                               // the window below takes its newest id from g, and no other word of it is the one just written
    }
    const unsigned n = tot < (unsigned long long)a.window ? (unsigned)tot : a.window;
    if (n < 2u) return;
    const unsigned base = (unsigned)((tot - n) & (DRY_MAX_WINDOW - 1u));
    for (unsigned i = tid; i < DRY_TABLE / 4u; i += DRY_NT) { key4[i] = uint4{DRY_NONE, DRY_NONE, DRY_NONE, DRY_NONE}; len4[i] = uint4{0u, 0u, 0u, 0u}; }
    for (unsigned i = tid; i < n; i += DRY_NT) h[i] = (!DEBUG && i == n - 1u) ? g : ring[(base + i) & (DRY_MAX_WINDOW - 1u)];
    if (tid == 0) { hits = 0u; count = 0u; }
    if (tid < DRY_MAX_MATCH) pen[tid] = a.pen[tid];
    __syncthreads();
    if (tid < DRY_MAX_MATCH) {                     // the tail, newest first; DRY_NONE ends a match: a breaker, or the window's start
        const unsigned v = tid < n ? h[n - 1u - tid] : DRY_NONE;
        bool brk = false;
        for (unsigned b = 0; b < a.n_breakers; b++) brk = brk || v == a.breakers[b];
        tail[tid] = brk ? DRY_NONE : v;
    }
    __syncthreads();
    const unsigned last = tail[0];
    if (last == DRY_NONE) return;                  // the whole workgroup: the newest id is a breaker
    for (unsigned j = tid; j + 1u < n; j += DRY_NT) {
        if (h[j] != last) continue;
        const unsigned cap = j + 1u < DRY_MAX_MATCH ? j + 1u : DRY_MAX_MATCH;      // j - k >= 0, and the cap
        unsigned m = 1u;
        while (m < cap && h[j - m] == tail[m]) m++;
        const unsigned t = h[j + 1u];
        for (unsigned i = t & (DRY_TABLE - 1u);; i = (i + 1u) & (DRY_TABLE - 1u)) {
            const unsigned old = atomicCAS(&key[i], DRY_NONE, t);
            if (old == DRY_NONE || old == t) { atomicMax(&len[i], m); break; }
        }
        hits = 1u;
    }
    __syncthreads();
    if (!hits) return;
    float *row = DEBUG ? nullptr : a.rows + (size_t)s * VOCAB;
    for (unsigned i = tid; i < DRY_TABLE; i += DRY_NT) {
        const unsigned t = key[i], l = len[i];
        if (t >= VOCAB || l < a.allowed) continue;                                  // (an empty key is >= V; the host has checked every id it planted)
        if (DEBUG) {
            const unsigned at = atomicAdd(&count, 1u);
            if (at < DRY_MAX_WINDOW) { a.dbg[1u + at] = t; a.dbg[1u + DRY_MAX_WINDOW + at] = l; }
        } else {
            row[t] = __fsub_rn(row[t], pen[l - a.allowed]);
        }
    }
    if (DEBUG) {
        __syncthreads();
        if (tid == 0) a.dbg[0] = count;
    }
}

} // namespace rwkvk
