// lookuptree.hip.h -- prompt-lookup decoding with DRAFT TREES as ONE device loop (gfx950, wave64): lookup.hip.h's loop with a drafter that keeps the
// `branches` most recent occurrences of the tail and merges what follows them into a trie, verified by the same pass with a parent per row.
// include/rwkv_mi355x.h rwkv_decode_lookup_trees has the contract.  No reference counterpart.
//
// A round is: k_lookup_tree_round, the checkpointing segmented pass (specseg.hip.h, unchanged), the row picks, k_specseg_accept, k_specseg_commit.  As in lookup.hip.h nothing is uploaded between rounds and the launch shape never changes: N segments of 1 + k rows.
//     k_lookup_tree_round<NT, W>  one workgroup per stream, four phases.
//         APPLY   lookup_apply (lookup.hip.h).
//         SEARCH  k_lookup_round's backward walk over windows of W starts (16-byte loads, a halo of 8 ids, the next window prefetched into registers),
//                 keeping the `branches` MOST RECENT matches.  Thread tid tests start p = i NT + tid at iteration i, so a wave's ballot IS word p / 64
//                 of the window's match bitmap: the four waves leave 16 words each in a 64-word LDS bitmap, no early exit inside a window.  Wave 0
//                 then holds one word per lane, scans the popcounts from the top word down (a suffix sum by shuffles) and every lane whose word is
//                 reached by the `need = branches - found` highest bits peels them off its word, highest first, into mstart[] at the rank the scan
//                 gave it: most recent first, within and across windows.  The walk ends when found == branches or the windows are exhausted.
//                 The rejection on the tail's last id stays in front: a miss costs one conflict-free LDS read.
//         TRIE    The continuations h[m_b + n : m_b + n + k], cut at len, are staged in LDS (8 x 32 words, one thread per word).  Wave 0 builds the
//                 trie LEVEL BY LEVEL, lane b = continuation b, which is engine.ngram_draft_tree's order: at level d the lanes that share (node
//                 reached, next id) elect their lowest lane (8 shuffles of one packed key); the leaders take node numbers count + rank in lane
//                 order while those are below k, the followers copy their leader's child, a lane whose leader got no node stops.
//                 THE CUT NEEDS NO RENUMBERING.  Nodes are created level by level, so depth is non-decreasing in the node index and a level never
//                 depends on a deeper one: the host loop's cut (depth <= remaining - 1) keeps a PREFIX of the nodes, which is exactly what building
//                 only the first min(k, remaining - 1) levels yields.  nd = the nodes those levels made.
//         WRITE   the segment's rows [id to feed, nd nodes, padding with id 0], their `from` bytes (the root for a node without a parent and for
//                 padding, else the parent's row) and the SpecSegEntry with the true n_draft.  A retired stream's rows and bytes stay as they are.
// Plain C++ and vector memory operations only; the one atomic is a vector atomic on the live count.  Nothing here writes host memory or waits.
#pragma once
#include "lookup.hip.h"

namespace rwkvk {

constexpr unsigned LKT_MAX_B = 8;                 // the most occurrences merged (RWKV_LOOKUP_MAX_BRANCHES)
constexpr unsigned LKT_ROW = 32;                  // words of a staged continuation: k <= SPEC_MAX_DRAFT = 31

struct LookupTreeArgs {
    LookupArgs l;                          // as k_lookup_round reads it
    unsigned char *from;                   // [rows of the pass] the row each row starts from (specseg.hip.h)
    int *parent;                           // the drafter alone: [N][k] the nodes' parents (-1: the root) INSTEAD of the from bytes, whose rows need
                                           // not fit a byte there; nullptr in the loop
    unsigned branches;
};

template <int NT, int W>
__global__ __launch_bounds__(NT) void k_lookup_tree_round(const LookupTreeArgs t)
{
    static_assert(NT % 64 == 0 && W % NT == 0 && W % 4 == 0 && LK_HALO % 4 == 0 && LK_HALO >= (int)LK_MAX_N - 1, "whole waves, whole 16-byte loads, a halo for the longest tail");
    static_assert(W / 64 == 64, "the window's match bitmap is one word per lane of a wave");
    static_assert(SPEC_MAX_DRAFT + 1 <= NT && SPEC_MAX_DRAFT < LKT_ROW && LKT_MAX_B * LKT_ROW <= NT, "one thread per row of a segment, one per staged id");
    constexpr int Q = (W + LK_HALO) / 4, QPT = (Q + NT - 1) / NT, SPT = W / NT;      // 16-byte pieces of a window, per thread; starts per thread
    __shared__ uint4 win[Q];
    __shared__ unsigned long long bits[W / 64];
    __shared__ unsigned mstart[LKT_MAX_B], cont[LKT_MAX_B][LKT_ROW], nid[LKT_ROW], s_found, s_nd;
    __shared__ int npar[LKT_ROW];
    const LookupArgs &g = t.l;
    const unsigned s = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, r0 = s * (g.k + 1u), n = g.n;
    const unsigned B = min(t.branches, LKT_MAX_B);
    LookupStream st = g.st[s];
    const SpecSegEntry prev = g.tab[s];
    unsigned *h = g.hist + st.off;

    lookup_apply(g, s, tid, prev, st, h);

    // ---- search: the B most recent earlier occurrences of the last n ids, most recent first
    const bool live = st.remain > 0u;
    const unsigned kd = live ? min(g.k, st.remain - 1u) : 0u;      // the levels the trie may have: k, cut at the depth the stream still wants
    unsigned found = 0u;
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
#pragma unroll 4
            for (int i = 0; i < SPT; i++) {
                const unsigned p = (unsigned)i * NT + tid;
                bool m = p < lim && ws[p + n - 1u] == rt[0];
                if (m) {
#pragma unroll
                    for (unsigned j = 1; j < LK_MAX_N; j++) if (j < n) m = m && ws[p + n - 1u - j] == rt[j];
                }
                const unsigned long long b = __ballot(m);
                if (lane == 0u) bits[p >> 6] = b;                  // word p / 64 of the window's bitmap
            }
            __syncthreads();
            if (tid < 64u) {
                unsigned long long word = bits[lane];
                const unsigned c = (unsigned)__popcll(word);
                unsigned incl = c;                                 // the matches in this word and every word above it
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) { const unsigned o = __shfl_down(incl, d); if (lane + (unsigned)d < 64u) incl += o; }
                const unsigned need = B - found, above = incl - c;
                for (unsigned r = above; r < need && word != 0ull; r++) {      // at most `need` <= 8 turns in one lane
                    const unsigned pos = 63u - (unsigned)__clzll((long long)word);
                    mstart[found + r] = base + lane * 64u + pos;
                    word &= ~(1ull << pos);
                }
                if (lane == 0u) s_found = min(B, found + incl);
            }
            __syncthreads();          // (also: every wave is done with `win` and `bits` before the next window lands)
            found = s_found;
            if (found == B) break;
        }
    }

    // ---- trie: stage the continuations, then wave 0 merges them level by level
    if (found > 0u) {
        const unsigned b = tid / LKT_ROW, d = tid % LKT_ROW;
        if (b < found) {
            const unsigned at = mstart[b] + n + d;
            if (d < g.k && at < st.len) cont[b][d] = h[at];
        }
    }
    __syncthreads();
    if (tid < 64u) {
        unsigned cnt = 0u;
        if (found > 0u) {
            const bool mine = lane < found;
            const unsigned clen = mine ? min(g.k, st.len - (mstart[mine ? lane : 0u] + n)) : 0u;
            int at = -1;
            bool alive = mine;
            for (unsigned d = 0; d < kd; d++) {
                const bool active = alive && d < clen;
                if (__ballot(active) == 0ull) break;
                const unsigned id = active ? cont[lane][d] : 0u;
                const unsigned long long key = active ? ((unsigned long long)(unsigned)(at + 1) << 32) | id : ~0ull;
                unsigned leader = lane;
#pragma unroll
                for (unsigned j = 0; j < LKT_MAX_B; j++) {
                    const unsigned long long other = __shfl(key, (int)j);
                    if (active && j < leader && other == key) leader = j;      // (ascending j and j < leader: the lowest lane that shares the key)
                }
                const bool lead = active && leader == lane;
                const unsigned long long lb = __ballot(lead);
                const unsigned node = cnt + (unsigned)__popcll(lb & ((1ull << lane) - 1ull));
                const int made = lead && node < g.k ? (int)node : -1;
                if (made >= 0) { nid[made] = id; npar[made] = at; }
                const int child = __shfl(made, (int)leader);
                if (active) { at = child; alive = child >= 0; }
                cnt = min(g.k, cnt + (unsigned)__popcll(lb));
            }
        }
        if (lane == 0u) s_nd = cnt;
    }
    __syncthreads();

    // ---- the segment's rows, where each starts from, and its table entry; a retired stream's rows stay as they are
    const unsigned nd = s_nd;
    if (live && tid <= g.k) {
        const bool node = tid >= 1u && tid <= nd;
        g.ids[r0 + tid] = tid == 0u ? h[st.len - 1u] : node ? nid[tid - 1u] : 0ull;
        const int par = node ? npar[tid - 1u] : -1;
        if (t.parent) { if (node) t.parent[(size_t)s * g.k + tid - 1u] = par; }
        else t.from[r0 + tid] = (unsigned char)(par < 0 ? r0 : r0 + 1u + (unsigned)par);
    }
    if (tid == 0) g.tab[s] = SpecSegEntry{r0, nd, s, live ? 1u : 0u};
}

} // namespace rwkvk
