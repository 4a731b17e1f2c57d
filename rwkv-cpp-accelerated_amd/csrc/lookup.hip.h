// lookup.hip.h -- prompt-lookup speculative decoding as ONE device loop (gfx950, wave64): the drafter and the bookkeeping of a round.
// include/rwkv_mi355x.h rwkv_decode_lookup_streams has the contract.  No reference counterpart.
//
// A round of the loop is: k_lookup_round, the checkpointing segmented pass (specseg.hip.h, unchanged), the row picks, k_specseg_accept,
// k_specseg_commit.  Nothing is uploaded between rounds: the round kernel PRODUCES what the pass reads (the ids of the rows, the segment table) and
// CONSUMES what the accept leaves (the records).  The launch shape never changes: N segments of 1 + k rows, stream s on slot s, rows s (k + 1) ..
//     k_lookup_round<NT, W>   one workgroup per stream.  APPLY the previous round's record (lookup_apply, which the tree form's round kernel shares): the
//                             accepted ids emitted[s][0 .. a - 1] and `next` go behind the stream's history and into its output row, its budget and
//                             counters move, a stream that has its ids RETIRES (table entry live = 0, the count of live streams falls: the accept
//                             gives such an entry a record that names no row, so the commit leaves its slot as it stood).  Then DRAFT: the up to kd = min(k, remaining - 1) ids behind the MOST RECENT earlier
//                             occurrence of the history's last n ids (engine.ngram_draft's rule, exactly), written as the segment's rows
//                             [id to feed, draft, padding] and its SpecSegEntry with the true n_draft.  The rows' `from` bytes never change -- row
//                             s (k + 1) itself, every other row the one in front -- and are the host's, written once.
// THE SEARCH.  Candidate starts are 0 .. len - n - 1 (something follows the occurrence; it may overlap the tail).  They are walked BACKWARDS in windows
// of W starts, aligned to W so that every load is 16 bytes wide and aligned: a window's W + 8 ids (the halo: n - 1 <= 7 ids of the next window, which
// a match that straddles the boundary reads) are staged in LDS by uint4 loads, and the NEXT window's loads are issued before the current one is
// tested, into registers, so a miss costs the test alone.  The tail lives in registers, newest id first.  A thread tests the starts p = i NT + tid
// (consecutive lanes, consecutive LDS words: no bank conflicts), i from high to low, on the tail's LAST id first -- one LDS read rejects nearly every
// start -- and a wave stops at the first i whose ballot is non-zero: its highest set lane is the wave's most recent match.  The waves' results meet in
// LDS, and the walk ends at the first window that holds a match: repetitive text finds it in the first.
// Plain C++ and vector memory operations only; the one atomic is a vector atomic on the live count.  Nothing here writes host memory or waits.
#pragma once
#include "specseg.hip.h"

namespace rwkvk {

constexpr int LK_NT = 256;                        // threads of a round's workgroup (four waves)
constexpr int LK_W = 4096;                        // candidate starts per window
constexpr int LK_HALO = 8;                        // ids staged behind a window: n - 1 <= 7, kept a multiple of 4 (16-byte loads)
constexpr unsigned LK_MAX_N = 8;                  // the longest tail (held in registers)
constexpr unsigned LK_NONE = 0xFFFFFFFFu;         // staged where the stream's buffer ends: no id

// one stream of a call: where its ids start in the history buffer (a multiple of 4) and how many fit (a multiple of 4: hist_len + n_tokens, rounded
// up), how many it holds, how many ids it still lacks (0: retired), and the counters the caller gets
struct LookupStream { unsigned long long off; unsigned cap, len, remain, rounds, drafted, accepted; };
static_assert(sizeof(LookupStream) == 32, "the host uploads and downloads the streams as 32-byte records");

struct LookupArgs {
    unsigned *hist;                    // every stream's ids, stream s at hist + st[s].off
    LookupStream *st;                  // [N]
    unsigned *out;                     // [N][n_tokens] what the streams emitted
    unsigned long long *live;          // the streams that still lack ids
    unsigned long long *ids;           // [N (k + 1)] the rows of the pass
    SpecSegEntry *tab;                 // [N] the pass's segment table; live = 1: the segment's stream was live when the entry was written
    const SpecSegRec *rec;             // [N] what the accept left of the previous round
    const unsigned long long *emitted; // [N][SPEC_MAX_DRAFT] the accepted ids of the previous round, in path order
    unsigned n_tokens, k, n;
};

// APPLY, the first phase of both round kernels (every thread of the workgroup calls it): what the previous round's accept left for stream s goes
// into st, behind its history h and into its output row -- nothing in front of the first round, nothing for a retired stream
__device__ __forceinline__ void lookup_apply(const LookupArgs &g, unsigned s, unsigned tid, const SpecSegEntry &prev, LookupStream &st, unsigned *h)
{
    if (!prev.live) return;
    const SpecSegRec rec = g.rec[s];
    const unsigned a = (unsigned)rec.a;
    if (a < st.remain && a <= SPEC_MAX_DRAFT && st.len + a + 1u <= st.cap) {      // (always: a <= the draft's depth <= remaining - 1, and cap >= hist_len + n_tokens)
        if (tid <= a) {
            const unsigned id = tid < a ? (unsigned)g.emitted[(size_t)s * SPEC_MAX_DRAFT + tid] : (unsigned)rec.next;
            h[st.len + tid] = id;
            g.out[(size_t)s * g.n_tokens + (g.n_tokens - st.remain) + tid] = id;
        }
        st.len += a + 1u; st.remain -= a + 1u; st.rounds += 1u; st.drafted += prev.n_draft; st.accepted += a;
    } else st.remain = 0u;
    __syncthreads();          // every thread has read g.st[s]; the appended ids are visible to the search
    if (tid == 0) {
        g.st[s] = st;
        if (st.remain == 0u) atomicAdd(g.live, ~0ull);
    }
}

template <int NT, int W>
__global__ __launch_bounds__(NT) void k_lookup_round(const LookupArgs g)
{
    static_assert(NT % 64 == 0 && W % NT == 0 && W % 4 == 0 && LK_HALO % 4 == 0 && LK_HALO >= (int)LK_MAX_N - 1, "whole waves, whole 16-byte loads, a halo for the longest tail");
    static_assert(SPEC_MAX_DRAFT + 1 <= NT, "one thread per row of a segment");
    constexpr int Q = (W + LK_HALO) / 4, QPT = (Q + NT - 1) / NT, SPT = W / NT;      // 16-byte pieces of a window, per thread; starts per thread
    __shared__ uint4 win[Q];
    __shared__ int wbest[NT / 64];
    const unsigned s = blockIdx.x, tid = threadIdx.x, r0 = s * (g.k + 1u), n = g.n;
    LookupStream st = g.st[s];
    const SpecSegEntry prev = g.tab[s];
    unsigned *h = g.hist + st.off;

    lookup_apply(g, s, tid, prev, st, h);

    // ---- draft: the most recent earlier occurrence of the last n ids
    const bool live = st.remain > 0u;
    const unsigned kd = live ? min(g.k, st.remain - 1u) : 0u;
    int best = -1;
    if (kd > 0u && st.len > n) {
        unsigned rt[LK_MAX_N];                                     // the tail, newest id first
#pragma unroll
        for (unsigned j = 0; j < LK_MAX_N; j++) rt[j] = j < n ? h[st.len - 1u - j] : 0u;
        const unsigned count = st.len - n;                         // the starts 0 .. count - 1
        const unsigned *ws = reinterpret_cast<const unsigned *>(win);
        uint4 nxt[QPT];
        auto fetch = [&](unsigned w) {
#pragma unroll
            for (int i = 0; i < QPT; i++) {
                const unsigned q = tid + i * NT, at = w * W + 4u * q;
                if (q < (unsigned)Q) nxt[i] = at + 4u <= st.cap ? *reinterpret_cast<const uint4 *>(h + at) : uint4{LK_NONE, LK_NONE, LK_NONE, LK_NONE};
            }
        };
        fetch((count - 1u) / W);
        for (int w = (int)((count - 1u) / W); w >= 0; w--) {
#pragma unroll
            for (int i = 0; i < QPT; i++) if (tid + i * NT < (unsigned)Q) win[tid + i * NT] = nxt[i];
            __syncthreads();
            if (w > 0) fetch((unsigned)w - 1u);                    // the next window travels while this one is tested
            const unsigned base = (unsigned)w * W, lim = min((unsigned)W, count - base);
            int mine = -1;
            for (int i = SPT - 1; i >= 0; i--) {
                const unsigned p = (unsigned)i * NT + tid;
                bool m = p < lim && ws[p + n - 1u] == rt[0];
                if (m) {
#pragma unroll
                    for (unsigned j = 1; j < LK_MAX_N; j++) if (j < n) m = m && ws[p + n - 1u - j] == rt[j];
                }
                const unsigned long long b = __ballot(m);
                if (b) { mine = (int)(base + (unsigned)i * NT + (tid & ~63u)) + 63 - __clzll((long long)b); break; }
            }
            if ((tid & 63u) == 0u) wbest[tid >> 6] = mine;
            __syncthreads();          // (also: every wave is done with `win` before the next window lands in it)
#pragma unroll
            for (int v = 0; v < NT / 64; v++) best = max(best, wbest[v]);
            if (best >= 0) break;
        }
    }

    // ---- the segment's rows and its table entry: [id to feed, draft, padding with a valid id]; a retired stream's rows stay as they are
    const unsigned nd = best >= 0 ? min(kd, st.len - ((unsigned)best + n)) : 0u;
    if (live && tid <= g.k) g.ids[r0 + tid] = tid == 0u ? h[st.len - 1u] : tid <= nd ? h[(unsigned)best + n + tid - 1u] : 0ull;
    if (tid == 0) g.tab[s] = SpecSegEntry{r0, nd, s, live ? 1u : 0u};
}

} // namespace rwkvk
