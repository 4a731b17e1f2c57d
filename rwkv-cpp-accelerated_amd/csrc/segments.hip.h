// segments.hip.h -- the SEGMENTED pass of the chunk path (gfx950, wave64): the rows of a pass are runs of consecutive tokens, each run on a state
// slot of its own.  include/rwkv_mi355x.h rwkv_forward_segments has the contract.  No reference counterpart: the reference knows
// n tokens of one sequence on slot 0 (GPT) or one token for each of n sequences (PARRALEL), which are the two ends of this layout.
//
// Only two places of a pass know which sequence a row belongs to -- the token shift of the LayerNorm sites and the state walk of the WKV kernel --
// and both read it from the ROW PLAN, [rows of the pass]{slot, flags} on the device: SEG_FIRST, the row is the first of its piece (its shift input
// and WKV state come from the slot); SEG_LAST, the last of its piece (its LayerNorm outputs and WKV state go to the slot).  A piece is what a pass
// holds of a segment.  Everything else of a pass (GEMMs, k_seq_resid, k_seq_stage<0>, k_seq_embed, the head) is row-independent and runs unchanged.
//     k_seg_site<NV>    k_seq_site's GPT arithmetic, expression for expression; a first row shifts from its slot, a last row's LayerNorm output
//                       goes to the STAGING rows [row][D] of the scratch set, not to the slot: the workgroups of a piece's last row would write
//                       what the workgroups of its first row read in the same launch
//     k_seg_wkv<TCAP>   k_seq_wkv's GPT walk with the same pinned roundings; the walk restarts from a slot's aa / bb at every first row (fetched
//                       into LDS by the (row, channel) threads in front of the barrier) and stores the running value at every last row.  It runs
//                       behind the K/V/R GEMM, so behind every read of the ln1 site: it COMMITS the staged xy rows to their slots
//     k_seg_stage<1>    k_seq_stage<1>; behind the ffn k/r GEMM, so behind every read of the ln2 site: it commits the staged dd rows
// A segmented pass so launches what a GPT pass of the same rows launches, and its GEMMs copy nothing (cp_n = 0).
// These are templates of their own, not further parameters of the seq.hip.h kernels, so that every instance the other paths launch keeps its name
// and its code; they are first named behind every other kernel (engine.hip seg_fns), which is where hipcc emits them.
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
    const int hh = t / SEQ_T, th = t % SEQ_T;
    const SegRow row = g.plan[t];
    const bool first = seg_first(row, t), last = (row.flags & SEG_LAST) != 0u;
    int c0, c1;
    octant_range(D, o, c0, c1);
    const bool lnprev = !first;      // the shift input is a LayerNorm output: of the previous row, or already stored (the slot)
    const double *xprow = first ? a.state_par + (size_t)row.slot * a.slot_stride : a.x + (size_t)(t - 1) * D;
    double mean, rstd, meanp, rstdp;
    seq_row_stats2(a.stat, t, lnprev ? t - 1 : t, D, mean, rstd, meanp, rstdp);
    if (!lnprev) { meanp = 0.0; rstdp = 1.0; }
    const int qd = (c0 >> 2) + threadIdx.x;
    const bool live = qd < (c1 >> 2);
    float v[NV][4];
    double So[NV];
    float amax[NV];
#pragma unroll
    for (int m = 0; m < NV; m++) { So[m] = 0.0; amax[m] = 0.f; v[m][0] = v[m][1] = v[m][2] = v[m][3] = 0.f; }
    if (live) {
        double xt[4], xp[4], lw[4], lb[4];
        load_quad_f64(a.x + (size_t)t * D, qd, xt);
        load_quad_f64(xprow, qd, xp);
        load_quad_f64(a.lnw, qd, lw);
        load_quad_f64(a.lnb, qd, lb);
        double xx[4], xprev[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            xx[e] = lw[e] * ((xt[e] - mean) * rstd) + lb[e];
            xprev[e] = lnprev ? lw[e] * ((xp[e] - meanp) * rstdp) + lb[e] : xp[e];
            if (last) g.stage[(size_t)t * D + qd * 4 + e] = xx[e];
        }
#pragma unroll
        for (int m = 0; m < NV; m++) {
            const f32x4 rr = reinterpret_cast<const f32x4 *>(a.r[m])[qd], oo = reinterpret_cast<const f32x4 *>(a.o[m])[qd];
            double mk[4];
            load_quad_f64(a.mix[m], qd, mk);
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const float f = (float)(xx[e] * mk[e] + xprev[e] * (1.0 - mk[e]));   // :339-343,:377-384
                v[m][e] = f * rr[e];
                So[m] += (double)(f * oo[e]);
                amax[m] = fmaxf(amax[m], fabsf(v[m][e]));
            }
        }
    }
    eblock_max<NV>(amax, red);
#pragma unroll
    for (int m = 0; m < NV; m++) {
        unsigned ls[3] = {0u, 0u, 0u};
        if (live) seq_store_quad(a.img[m] + hh * a.img_h, qd, th, v[m], inv_scale(amax[m]), ls);
        seq_finish(ls, So[m], c1 - c0, amax[m], a.part + hh * a.part_h + ((size_t)m * SEQ_T + th) * SEQ_O + o, red);
    }
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
            const int CB = (a.D + 15) >> 4, hh = t / SEQ_T, th = t % SEQ_T;
            const float *pk = a.pk + hh * a.pk_h;
            const SeqPart *qp = a.qpart + hh * a.part_h;
            const size_t so = (size_t)row.slot * a.slot_stride + i;
            // a piece's start state, every first row at once: the serial walk below reads LDS only
            if (row.flags & SEG_FIRST) { aa0[t][ch] = a.saa[so]; aas[t][ch] = a.sbb[so]; }
            const float k = seq_val(pk, 3 * CB, 0 * CB + (i >> 4), th, i & 15, seq_so(qp, 0, th));
            const float v = seq_val(pk, 3 * CB, 1 * CB + (i >> 4), th, i & 15, seq_so(qp, 1, th));
            const float r = seq_val(pk, 3 * CB, 2 * CB + (i >> 4), th, i & 15, seq_so(qp, 2, th));
            e1s[t][ch] = exp(a.uw[i] + (double)k);
            eks[t][ch] = exp((double)k);
            vs[t][ch] = (double)v;
            sgs[t][ch] = 1.0 / (1.0 + (double)expf(-r));       // rwkv.cu:250: exp of a float argument
            // the commit of the ln1 site's last rows: every workgroup of that site and of the K/V/R GEMM behind it is done
            if (row.flags & SEG_LAST) g.sxy[so] = g.stage[(size_t)t * a.D + i];
        }
    }
    __syncthreads();
    // k_seq_wkv's GPT walk, one thread per channel along the rows of the pass, the steps' roundings pinned as there (one fma and one product for aa,
    // one sum and one product for bb): the state after a row must not depend on what else the pass holds
    if (threadIdx.x < WKV_CH && i < a.D) {
        double aa = 0.0, bb = 0.0;
        const double ew = a.ew[i];
        for (int tt = 0; tt < a.T; tt++) {
#pragma clang fp contract(off)
            const SegRow row = rows[tt];
            if (row.flags & SEG_FIRST) { aa = aa0[tt][ch]; bb = aas[tt][ch]; }
            const double ek = eks[tt][ch], vv = vs[tt][ch];
            eks[tt][ch] = aa;                 // state before row tt (the slot of e^k is free once read)
            aas[tt][ch] = bb;
            aa = __builtin_fma(ek, vv, aa) * ew;
            bb = (bb + ek) * ew;
            if (row.flags & SEG_LAST) {       // (stores do not hold the walk up)
                const size_t so = (size_t)row.slot * a.slot_stride + i;
                a.saa[so] = aa; a.sbb[so] = bb;
            }
        }
    }
    __syncthreads();
    if (live) {
        const double e1 = e1s[t][ch];
        a.y[(size_t)t * a.D + i] = (float)(sgs[t][ch] * ((eks[t][ch] + e1 * vs[t][ch]) / (aas[t][ch] + e1)));
    }
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
// k_seq_stage<KIND> (KIND 1: relu(k)^2 of the ffn k GEMM -> the ffn_v input) with the commit of the ln2 site's last rows in front: workgroup
// (row, octant) copies octant o of D of its row, if the row is a last one
template <int KIND>
__global__ __launch_bounds__(SEQ_ENT) void k_seg_stage(SegStageArgs g)
{
    static_assert(KIND == 1, "the stage kernel behind the ffn k/r GEMM");
    __shared__ double red[SEQ_ENW * 4];
    const SeqStageArgs &a = g.s;
    RWKV_ARGS_NOW(g.plan, g.stage, g.sdd);      // (see k_seq_resid)
    RWKV_ARGS_NOW(a.pk, a.qpart_k, a.r, a.o, a.img, a.part);
    const int K = a.K, tg = blockIdx.x / SEQ_O, o = blockIdx.x % SEQ_O;
    const int hh = tg / SEQ_T, t = tg % SEQ_T;
    const SegRow row = g.plan[tg];
    if (row.flags & SEG_LAST) {
        int d0, d1;
        octant_range(g.D, o, d0, d1);
        for (int j = d0 + threadIdx.x; j < d1; j += SEQ_ENT) g.sdd[(size_t)row.slot * g.slot_stride + j] = g.stage[(size_t)tg * g.D + j];
    }
    const float *pk = a.pk + hh * a.pk_h;
    int c0, c1;
    octant_range(K, o, c0, c1);
    const float sok = seq_so(a.qpart_k + hh * a.partk_h, 0, t);
    const int q0 = c0 >> 2, q1 = c1 >> 2;
    float v[SEQ_SQ][4];
    double So = 0.0;
    float am[1] = {0.f};
#pragma unroll
    for (int i = 0; i < SEQ_SQ; i++) {
        const int qd = q0 + threadIdx.x + i * SEQ_ENT;
        v[i][0] = v[i][1] = v[i][2] = v[i][3] = 0.f;
        if (qd < q1) {
            float f[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int CB = ((K >> 2) + 15) >> 4;
                float k = seq_val(pk, 5 * CB, e * CB + (qd >> 4), t, qd & 15, sok);   // hidden units 4 qd .. 4 qd + 3 = classes 0..3 of channel qd
                k = k * (float)(k > 0.f);
                f[e] = k * k;                                                          // relu(k)^2, rwkv.cu:189-190
            }
            const f32x4 rv = reinterpret_cast<const f32x4 *>(a.r)[qd], ov = reinterpret_cast<const f32x4 *>(a.o)[qd];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                v[i][e] = f[e] * rv[e];
                So += (double)(f[e] * ov[e]);
                am[0] = fmaxf(am[0], fabsf(v[i][e]));
            }
        }
    }
    eblock_max<1>(am, red);
    const float inv_s = inv_scale(am[0]);
    unsigned ls[3] = {0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < SEQ_SQ; i++) {
        const int qd = q0 + threadIdx.x + i * SEQ_ENT;
        if (qd < q1) seq_store_quad(a.img + hh * a.img_h, qd, t, v[i], inv_s, ls);
    }
    seq_finish(ls, So, c1 - c0, am[0], a.part + hh * a.part_h + (size_t)t * SEQ_O + o, red);
}

} // namespace rwkvk
