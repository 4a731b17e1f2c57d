// specseg.hip.h -- speculative greedy decoding for MANY streams (gfx950, wave64): the CHECKPOINTING SEGMENTED pass of the chunk path and the commit
// of what stands, per segment.  include/rwkv_mi355x.h rwkv_spec_verify_segments has the contract.  No reference counterpart.
//
// The pass is a segmented pass (segments.hip.h: the rows are runs of consecutive tokens, each run on a state slot of its own, as the ROW PLAN says)
// that commits NOTHING, like the verify pass of one stream (spec.hip.h): it leaves, per layer and row, what the row's slot holds once that row is
// the last one fed -- ckpt[which][l][t][D] f64, which = 0 xy, 1 aa, 2 bb, 3 dd.  One pass of up to 64 rows, never cut: a verify knows what stands
// only behind the head.  Of the plan only SEG_FIRST is read: no row is a last one before the accept kernel has said so.
//     k_specseg_site<NV>    a first row shifts from its slot, every row's LayerNorm output goes to the checkpoint rows; no slot, no staging row is written
//     k_specseg_wkv<TCAP>   the walk restarts from a slot's aa / bb at every first row and leaves the state after EVERY row in two LDS tables, which the
//                           (row, channel) threads store to the checkpoint arrays; no slot is written
//     k_specseg_accept      one wave per segment: the first draft id the picks do not confirm; the record {a, next, row}
//     k_specseg_commit      grid (L D / 2, segment): xy, aa, bb, dd of the segment's slot from the checkpoint row that stands, 16 bytes per load and store
// The ffn side runs the plain k_seq_stage<1>: there is nothing to commit behind the ffn k/r GEMM.  The arithmetic is seq.hip.h's (seq_site_row,
// seq_wkv_terms / seq_wkv_step / seq_wkv_out); the kernels are templates of their own, first named behind every other kernel (engine.hip specseg_fns).
// Plain C++ and vector memory operations only; nothing here writes host memory or waits for anything.
#pragma once
#include "segments.hip.h"
#include "spec.hip.h"

namespace rwkvk {

// ------------------------------------------------------------------------------------------
// s: as k_seq_site reads it, with s.state_par = this layer's xy / dd of slot 0, s.slot_stride = L D and s.ckpt = this site's checkpoint rows [T][D]
struct SpecSegSiteArgs {
    SeqSiteArgs s;
    const SegRow *plan;          // [T] of the pass
};
template <int NV>
__global__ __launch_bounds__(SEQ_ENT) void k_specseg_site(SpecSegSiteArgs g)
{
    static_assert(NV == 2 || NV == 3, "the sites with a token shift: ln1 (3 vectors) and ln2 (2)");
    __shared__ double red[SEQ_ENW * 4];
    const SeqSiteArgs &a = g.s;
    RWKV_ARGS_NOW(g.plan, a.ckpt, a.x, a.stat, a.lnw, a.lnb, a.state_par, a.part);      // (see k_seq_resid)
    RWKV_ARGS_NOW(a.mix[0], a.r[0], a.o[0], a.img[0]);
    RWKV_ARGS_NOW(a.mix[NV - 1], a.r[NV - 1], a.o[NV - 1], a.img[NV - 1], a.mix[NV > 2 ? 1 : 0], a.r[NV > 2 ? 1 : 0], a.o[NV > 2 ? 1 : 0], a.img[NV > 2 ? 1 : 0]);
    const int D = a.D, t = blockIdx.x / SEQ_O, o = blockIdx.x % SEQ_O;      // t: row of the pass (0 .. 63)
    const SegRow row = g.plan[t];
    const bool first = seg_first(row, t);
    const double *xprow = first ? a.state_par + (size_t)row.slot * a.slot_stride : a.x + (size_t)(t - 1) * D;
    double *ck = a.ckpt + (size_t)t * D;
    seq_site_row<NV>(a, t, o, true, !first, xprow, [&](int j, const double (&xx)[4]) {
        reinterpret_cast<f64x2 *>(ck + j)[0] = f64x2{xx[0], xx[1]};
        reinterpret_cast<f64x2 *>(ck + j)[1] = f64x2{xx[2], xx[3]};
    }, red);
}

// ------------------------------------------------------------------------------------------
// w: as k_seq_wkv reads it, with w.saa / w.sbb = this layer's aa / bb of slot 0 (read only), w.slot_stride = L D and w.ckpt_aa / w.ckpt_bb = this
// layer's checkpoint rows [T][D] (w.par, w.slot0 unused)
struct SpecSegWkvArgs {
    SeqWkvArgs w;
    const SegRow *plan;          // [T] of the pass
};
// WHERE THE STATE AFTER EACH ROW IS KEPT.  The one-stream verify (k_seq_wkv<32, true>) reads it off the walk's own tables: the state before row t + 1
// IS the state after row t, so one extra table row is all it adds.  A restart breaks that: in front of a first row the tables hold the slot's start
// state, and the state after the row before it is nowhere.  Here the walk writes the state after row t into two tables of its own: aa into aa0[t] --
// the table the pieces' start aa waits in, whose row t the walk has read (a first row) or never needed (any other) by the time it has stepped over
// row t -- and bb into bbn[t], the one table this kernel adds to k_seg_wkv's.  Two LDS stores per step, no branch, nothing global on the serial
// thread; the TCAP x 16 threads then store both tables to the checkpoint arrays in rows of 128 bytes.
// LDS: seven [TCAP][16] f64 tables and the rows' first flags: 28 800 bytes at TCAP = 32, 57 600 (56.25 KB) at 64 (static limit 64 KB; two workgroups
// of 16 waves fit a CU's 160 KB, which is what its 32 wave slots hold anyway).  A walk that stored to the checkpoint arrays itself would need six tables (49 KB), but
// puts 2 x 64 global stores with their address arithmetic into the one serial wave that everything else waits for.
template <int TCAP>
__global__ __launch_bounds__(TCAP * WKV_CH) void k_specseg_wkv(SpecSegWkvArgs g)
{
    __shared__ double e1s[TCAP][WKV_CH], eks[TCAP][WKV_CH], vs[TCAP][WKV_CH], sgs[TCAP][WKV_CH], aas[TCAP][WKV_CH], aa0[TCAP][WKV_CH], bbn[TCAP][WKV_CH];
    __shared__ unsigned firsts[TCAP];
    const SeqWkvArgs &a = g.w;
    RWKV_ARGS_NOW(g.plan, a.ckpt_aa, a.ckpt_bb);      // (see k_seq_resid)
    RWKV_ARGS_NOW(a.pk, a.qpart, a.uw, a.ew, a.saa, a.sbb, a.y);
    const int ch = threadIdx.x & (WKV_CH - 1), t = threadIdx.x / WKV_CH;     // t: row of the pass
    const int i = blockIdx.x * WKV_CH + ch;
    const bool live = i < a.D && t < a.T;
    if (t < a.T) {
        const SegRow row = g.plan[t];
        const bool first = seg_first(row, t);
        if (ch == 0) firsts[t] = first ? 1u : 0u;
        if (live) {
            // a piece's start state, every first row at once: the serial walk below reads and writes LDS only
            if (first) { const size_t so = (size_t)row.slot * a.slot_stride + i; aa0[t][ch] = a.saa[so]; aas[t][ch] = a.sbb[so]; }
            seq_wkv_terms(a, t, i, e1s[t][ch], eks[t][ch], vs[t][ch], sgs[t][ch]);
        }
    }
    __syncthreads();
    if (threadIdx.x < WKV_CH && i < a.D) {
        double aa = 0.0, bb = 0.0;
        const double ew = a.ew[i];
        for (int tt = 0; tt < a.T; tt++) {
            if (firsts[tt]) { aa = aa0[tt][ch]; bb = aas[tt][ch]; }
            seq_wkv_step(aa, bb, eks[tt][ch], vs[tt][ch], aas[tt][ch], ew);
            aa0[tt][ch] = aa; bbn[tt][ch] = bb;       // the state after row tt (aa0[tt] is free: read just above, or never needed)
        }
    }
    __syncthreads();
    if (live) {
        a.y[(size_t)t * a.D + i] = seq_wkv_out(e1s[t][ch], sgs[t][ch], eks[t][ch], vs[t][ch], aas[t][ch]);
        a.ckpt_aa[(size_t)t * a.D + i] = aa0[t][ch];
        a.ckpt_bb[(size_t)t * a.D + i] = bbn[t][ch];
    }
}

// ------------------------------------------------------------------------------------------
// one entry per segment, uploaded with the ids and the plan: the segment's last CERTAIN row r0 + c (its pick is the first one a draft id is held
// to), the number of draft rows behind it, and the slot
struct SpecSegEntry { unsigned rc, n_draft, slot, pad; };
struct SpecSegRec { unsigned long long a, next, row; };      // what stands of segment i: the host's download, and what the commit reads
struct SpecSegAcceptArgs {
    const unsigned long long *ids;         // [T] the ids the pass was fed
    const unsigned long long *pick;        // [T] the picks of the rows
    const SpecSegEntry *tab;               // [n_segs]
    SpecSegRec *rec;                       // [n_segs]
};
// One wave per segment (blockIdx.x), one lane per draft id: a = the number of leading j with ids[rc + 1 + j] == pick[rc + j].  Row rc + a is the last
// row that was fed rightly; its pick is the id that follows.
template <unsigned NT> __global__ __launch_bounds__(NT) void k_specseg_accept(const SpecSegAcceptArgs g)
{
    static_assert(NT == 64 && SPEC_MAX_DRAFT < NT, "one wave, one lane per draft id");
    const SpecSegEntry e = g.tab[blockIdx.x];
    const unsigned j = threadIdx.x;
    const bool miss = j >= e.n_draft || g.ids[e.rc + 1 + j] != g.pick[e.rc + j];      // (lane n_draft and the lanes behind it always miss: a <= n_draft)
    const unsigned long long m = __ballot(miss);
    const unsigned acc = (unsigned)__ffsll((long long)m) - 1u;
    if (j == acc) g.rec[blockIdx.x] = SpecSegRec{acc, g.pick[e.rc + acc], e.rc + acc};
}

struct SpecSegCommitArgs {
    const SpecSegRec *rec;                 // k_specseg_accept's records
    const SpecSegEntry *tab;
    const double *ckpt;                    // [4][L][rows][D]
    double *xy, *aa, *bb, *dd;             // slot 0 of the four state arrays; a slot is L D doubles
    unsigned L, D, rows;                   // rows of the pass
};
// grid (pairs of L D, segment): the slot of segment blockIdx.y from checkpoint row rec.row.  D is a multiple of 64: a pair never straddles two layers.
template <int NT> __global__ __launch_bounds__(NT) void k_specseg_commit(const SpecSegCommitArgs g)
{
    const size_t LD = (size_t)g.L * g.D, e = ((size_t)blockIdx.x * NT + threadIdx.x) * 2;
    if (e >= LD) return;
    const unsigned long long row = g.rec[blockIdx.y].row;
    if (row >= g.rows) return;             // (never: k_specseg_accept writes rc + a < rows)
    const size_t l = e / g.D, j = e - l * g.D, arr = LD * g.rows, src = (l * g.rows + (size_t)row) * g.D + j;
    const size_t dst = (size_t)g.tab[blockIdx.y].slot * LD + e;
    const f64x2 xy = *reinterpret_cast<const f64x2 *>(g.ckpt + src), aa = *reinterpret_cast<const f64x2 *>(g.ckpt + arr + src);
    const f64x2 bb = *reinterpret_cast<const f64x2 *>(g.ckpt + 2 * arr + src), dd = *reinterpret_cast<const f64x2 *>(g.ckpt + 3 * arr + src);
    *reinterpret_cast<f64x2 *>(g.xy + dst) = xy; *reinterpret_cast<f64x2 *>(g.aa + dst) = aa;
    *reinterpret_cast<f64x2 *>(g.bb + dst) = bb; *reinterpret_cast<f64x2 *>(g.dd + dst) = dd;
}

} // namespace rwkvk
