// segments.hip.h -- the SEGMENTED pass of the chunk path (gfx950, wave64): the rows of a pass are runs of consecutive tokens, each run on a state
// slot of its own.  include/rwkv_mi355x.h rwkv_forward_segments has the contract.  No reference counterpart: the reference knows
// n tokens of one sequence on slot 0 (GPT) or one token for each of n sequences (PARRALEL), which are the two ends of this layout.
//
// Only two places of a pass know which sequence a row belongs to -- the token shift of the LayerNorm sites and the state walk of the WKV kernel --
// and both read it from the ROW PLAN, [rows of the pass]{slot, flags} on the device: SEG_FIRST, the row is the first of its piece (its shift input
// and WKV state come from the slot); SEG_LAST, the last of its piece (its LayerNorm outputs and WKV state go to the slot).  A piece is what a pass
// holds of a segment.  Everything else of a pass (GEMMs, k_seq_resid, k_seq_stage<0>, k_seq_embed, the head) is row-independent and runs unchanged.
// The arithmetic is seq.hip.h's, written there once (seq_site_row, seq_wkv_terms / seq_wkv_step / seq_wkv_out, seq_stage_row); a kernel here holds
// only what the plan decides:
//     k_seg_site<NV>    a first row shifts from its slot, a last row's LayerNorm output goes to the STAGING rows [row][D] of the scratch set, not
//                       to the slot: the workgroups of a piece's last row would write what the workgroups of its first row read in the same launch
//     k_seg_wkv<TCAP>   the walk restarts from a slot's aa / bb at every first row (fetched into LDS by the (row, channel) threads in front of the
//                       barrier) and stores the running value at every last row.  It runs behind the K/V/R GEMM, so behind every read of the ln1
//                       site: it COMMITS the staged xy rows to their slots
//     k_seg_stage<1>    behind the ffn k/r GEMM, so behind every read of the ln2 site: it commits the staged dd rows
// A segmented pass so launches what a GPT pass of the same rows launches, and its GEMMs copy nothing (cp_n = 0).
// The kernels are templates of their own, not further parameters of the seq.hip.h kernels: every instance the other paths launch keeps its name and
// none carries the plan's branches.  They are first named behind every other kernel (engine.hip seg_fns), which is where hipcc emits them.
// Plain C++ and vector memory operations only.
#pragma once
#include "seq.hip.h"

namespace rwkvk {

struct SegRow { unsigned slot, flags; };
constexpr unsigned SEG_FIRST = 1u, SEG_LAST = 2u;
// row 0 of a pass is always the first of a piece (the validator writes it so; a plan that did not would send the shift to row -1)
__device__ __forceinline__ bool seg_first(const SegRow &r, int t) { return (r.flags & SEG_FIRST) != 0u || t == 0; }

// ------------------------------------------------------------------------------------------
// s: as k_seq_site reads it, with s.state_par = this layer's xy / dd of slot 0 and s.slot_stride = L D (s.state, s.state_new, s.par, s.slot0, s.ckpt unused)
struct SegSiteArgs {
    SeqSiteArgs s;
    const SegRow *plan;          // [T] of this pass
    double *stage;               // [T][D]: the LayerNorm output of the last rows, until the commit
};
template <int NV>
__global__ __launch_bounds__(SEQ_ENT) void k_seg_site(SegSiteArgs g)
{
    static_assert(NV == 2 || NV == 3, "the sites with a token shift: ln1 (3 vectors) and ln2 (2)");
    __shared__ double red[SEQ_ENW * 4];
    const SeqSiteArgs &a = g.s;
    RWKV_ARGS_NOW(g.plan, g.stage, a.x, a.stat, a.lnw, a.lnb, a.state_par, a.part);      // (see k_seq_resid)
    RWKV_ARGS_NOW(a.mix[0], a.r[0], a.o[0], a.img[0]);
    RWKV_ARGS_NOW(a.mix[NV - 1], a.r[NV - 1], a.o[NV - 1], a.img[NV - 1], a.mix[NV > 2 ? 1 : 0], a.r[NV > 2 ? 1 : 0], a.o[NV > 2 ? 1 : 0], a.img[NV > 2 ? 1 : 0]);
    const int D = a.D, t = blockIdx.x / SEQ_O, o = blockIdx.x % SEQ_O;      // t: row of the pass (0 .. 63)
    const SegRow row = g.plan[t];
    const bool first = seg_first(row, t), last = (row.flags & SEG_LAST) != 0u;
    // a first row shifts from its slot (a LayerNorm output already stored), every other row from the row before it
    const double *xprow = first ? a.state_par + (size_t)row.slot * a.slot_stride : a.x + (size_t)(t - 1) * D;
    seq_site_row<NV>(a, t, o, true, !first, xprow, [&](int j, const double (&xx)[4]) {
        if (last)
#pragma unroll
            for (int e = 0; e < 4; e++) g.stage[(size_t)t * D + j + e] = xx[e];
    }, red);
}

// ------------------------------------------------------------------------------------------
// w: as k_seq_wkv reads it, with w.saa / w.sbb = this layer's aa / bb of slot 0 and w.slot_stride = L D (w.par, w.slot0, w.ckpt_* unused)
struct SegWkvArgs {
    SeqWkvArgs w;
    const SegRow *plan;          // [T] of this pass
    const double *stage;         // [T][D]: the ln1 site's staged rows ...
    double *sxy;                 // ... and where they go: this layer's xy of slot 0
};
// LDS: k_seq_wkv's five [TCAP][16] f64 tables, one more for the aa a piece starts from (its bb waits in aas[t], which the walk overwrites with the
// same value), and the plan's rows: 24.5 KB at TCAP = 32, 49 KB at 64 (static limit 64 KB).
template <int TCAP>
__global__ __launch_bounds__(TCAP * WKV_CH) void k_seg_wkv(SegWkvArgs g)
{
    __shared__ double e1s[TCAP][WKV_CH], eks[TCAP][WKV_CH], vs[TCAP][WKV_CH], sgs[TCAP][WKV_CH], aas[TCAP][WKV_CH], aa0[TCAP][WKV_CH];
    __shared__ SegRow rows[TCAP];
    const SeqWkvArgs &a = g.w;
    RWKV_ARGS_NOW(g.plan, g.stage, g.sxy);      // (see k_seq_resid)
    RWKV_ARGS_NOW(a.pk, a.qpart, a.uw, a.ew, a.saa, a.sbb, a.y);
    const int ch = threadIdx.x & (WKV_CH - 1), t = threadIdx.x / WKV_CH;     // t: row of the pass
    const int i = blockIdx.x * WKV_CH + ch;
    const bool live = i < a.D && t < a.T;
    if (t < a.T) {
        SegRow row = g.plan[t];
        if (seg_first(row, t)) row.flags |= SEG_FIRST;
        if (ch == 0) rows[t] = row;
        if (live) {
            const size_t so = (size_t)row.slot * a.slot_stride + i;
            // a piece's start state, every first row at once: the serial walk below reads LDS only
            if (row.flags & SEG_FIRST) { aa0[t][ch] = a.saa[so]; aas[t][ch] = a.sbb[so]; }
            seq_wkv_terms(a, t, i, e1s[t][ch], eks[t][ch], vs[t][ch], sgs[t][ch]);
            // the commit of the ln1 site's last rows: every workgroup of that site and of the K/V/R GEMM behind it is done
            if (row.flags & SEG_LAST) g.sxy[so] = g.stage[(size_t)t * a.D + i];
        }
    }
    __syncthreads();
    // one thread per channel along the rows of the pass: the walk restarts from LDS at every first row and stores the running value at every last
    if (threadIdx.x < WKV_CH && i < a.D) {
        double aa = 0.0, bb = 0.0;
        const double ew = a.ew[i];
        for (int tt = 0; tt < a.T; tt++) {
            const SegRow row = rows[tt];
            if (row.flags & SEG_FIRST) { aa = aa0[tt][ch]; bb = aas[tt][ch]; }
            seq_wkv_step(aa, bb, eks[tt][ch], vs[tt][ch], aas[tt][ch], ew);
            if (row.flags & SEG_LAST) {       // (stores do not hold the walk up)
                const size_t so = (size_t)row.slot * a.slot_stride + i;
                a.saa[so] = aa; a.sbb[so] = bb;
            }
        }
    }
    __syncthreads();
    if (live) a.y[(size_t)t * a.D + i] = seq_wkv_out(e1s[t][ch], sgs[t][ch], eks[t][ch], vs[t][ch], aas[t][ch]);
}

// ------------------------------------------------------------------------------------------
struct SegStageArgs {
    SeqStageArgs s;              // as k_seq_stage<1> reads it
    const SegRow *plan;          // [T] of this pass
    const double *stage;         // [T][D]: the ln2 site's staged rows ...
    double *sdd;                 // ... and where they go: this layer's dd of slot 0
    size_t slot_stride;          // L D
    int D;
};
// the commit of the ln2 site's last rows -- workgroup (row, octant) copies octant o of D of its row, if the row is a last one -- in front of
// k_seq_stage<KIND>'s body (KIND 1: relu(k)^2 of the ffn k GEMM -> the ffn_v input)
template <int KIND>
__global__ __launch_bounds__(SEQ_ENT) void k_seg_stage(SegStageArgs g)
{
    static_assert(KIND == 1, "the stage kernel behind the ffn k/r GEMM");
    __shared__ double red[SEQ_ENW * 4];
    const SeqStageArgs &a = g.s;
    RWKV_ARGS_NOW(g.plan, g.stage, g.sdd);      // (see k_seq_resid)
    RWKV_ARGS_NOW(a.pk, a.qpart_k, a.r, a.o, a.img, a.part);
    const int tg = blockIdx.x / SEQ_O, o = blockIdx.x % SEQ_O;
    const SegRow row = g.plan[tg];
    if (row.flags & SEG_LAST) {
        int d0, d1;
        octant_range(g.D, o, d0, d1);
        for (int j = d0 + threadIdx.x; j < d1; j += SEQ_ENT) g.sdd[(size_t)row.slot * g.slot_stride + j] = g.stage[(size_t)tg * g.D + j];
    }
    seq_stage_row<KIND>(a, tg, o, red);
}

} // namespace rwkvk
