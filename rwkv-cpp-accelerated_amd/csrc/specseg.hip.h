// specseg.hip.h -- speculative decoding for MANY streams (gfx950, wave64): the CHECKPOINTING SEGMENTED pass of the chunk path with a PARENT per row, the
// accept of the one path that stands per segment, and the commit of exactly that.  include/rwkv_mi355x.h rwkv_spec_verify_segments and
// rwkv_spec_verify_trees have the contract.  No reference counterpart.
//
// The pass is a segmented pass (segments.hip.h: the rows are runs of tokens, each run on a state slot of its own, as the ROW PLAN says) that commits
// NOTHING, like the verify pass of one stream (spec.hip.h): it leaves, per layer and row, what the row's slot holds once that row is the last one fed
// -- ckpt[which][l][t][D] f64, which = 0 xy, 1 aa, 2 bb, 3 dd.  One pass of up to 64 rows, never cut: a verify knows what stands only behind the head.
// Of the plan only SEG_FIRST is read: no row is a last one before the accept kernel has said so.
// A segment's certain rows are a chain; its draft rows are a tree rooted at the last certain row, in topological order.  The device sees one table
// beside the row plan, from[T]: the row of the PASS whose state row t starts from -- the row in front for a certain row, the parent for a draft row, the
// row ITSELF for a first row (which starts from its slot).  A draft that is a chain is the case from[t] = t - 1.  RWKV has no cache to fork: the state
// behind every row is checkpointed per row anyway, so a branch is one more index.
//     k_specseg_site<NV>    a first row shifts from its slot, every other row from row from[t] (either half of the pass), its LayerNorm by that row's
//                           statistics; every row's LayerNorm output goes to the checkpoint rows; no slot, no staging row is written
//     k_specseg_wkv<TCAP>   the walk steps over the rows in order, starts each from the state after row from[t] (a first row: from its slot's aa / bb) and
//                           leaves the state after EVERY row in two LDS tables, which the (row, channel) threads store to the checkpoint arrays; no slot
//                           is written
//     k_specseg_accept      one wave per segment, lane j = draft row j: the rows whose every ancestor the picks confirm, by ballots; the record
//                           {a, next, row} and the accepted ids in path order.  A retired entry (live == 0) gets a record that names no row
//     k_specseg_commit      grid (L D / 2, segment): xy, aa, bb, dd of the segment's slot from the checkpoint row that stands, 16 bytes per load and store
// The ffn side runs the plain k_seq_stage<1>: there is nothing to commit behind the ffn k/r GEMM.  The arithmetic is seq.hip.h's (seq_site_row_from,
// seq_wkv_terms / seq_wkv_step / seq_wkv_out); the kernels are templates of their own, first named behind every other kernel (engine.hip specseg_fns).
// Plain C++ and vector memory operations only; nothing here writes host memory or waits for anything.
#pragma once
#include "segments.hip.h"
#include "spec.hip.h"

namespace rwkvk {

// ------------------------------------------------------------------------------------------
// s: as k_seq_site reads it, with s.state_par = this layer's xy / dd of slot 0, s.slot_stride = L D and s.ckpt = this site's checkpoint rows [T][D];
// from: [T] of the pass (see above), every entry <= its own row
struct SpecSegSiteArgs {
    SeqSiteArgs s;
    const SegRow *plan;          // [T] of the pass
    const unsigned char *from;
};
template <int NV>
__global__ __launch_bounds__(SEQ_ENT) void k_specseg_site(SpecSegSiteArgs g)
{
    static_assert(NV == 2 || NV == 3, "the sites with a token shift: ln1 (3 vectors) and ln2 (2)");
    __shared__ double red[SEQ_ENW * 4];
    const SeqSiteArgs &a = g.s;
    RWKV_ARGS_NOW(g.plan, g.from, a.ckpt, a.x, a.stat, a.lnw, a.lnb, a.state_par);      // (see k_seq_resid)
    RWKV_ARGS_NOW(a.part, a.mix[0], a.r[0], a.o[0], a.img[0]);
    RWKV_ARGS_NOW(a.mix[NV - 1], a.r[NV - 1], a.o[NV - 1], a.img[NV - 1], a.mix[NV > 2 ? 1 : 0], a.r[NV > 2 ? 1 : 0], a.o[NV > 2 ? 1 : 0], a.img[NV > 2 ? 1 : 0]);
    const int D = a.D, t = blockIdx.x / SEQ_O, o = blockIdx.x % SEQ_O;      // t: row of the pass (0 .. 63)
    const SegRow row = g.plan[t];
    const bool first = seg_first(row, t);
    const int tp = min((int)g.from[t], t);      // (the host's table never exceeds t: the clamp keeps a wrong one inside the pass)
    const double *xprow = first ? a.state_par + (size_t)row.slot * a.slot_stride : a.x + (size_t)tp * D;
    double *ck = a.ckpt + (size_t)t * D;
    seq_site_row_from<NV>(a, t, tp, o, true, !first, xprow, [&](int j, const double (&xx)[4]) {
        reinterpret_cast<f64x2 *>(ck + j)[0] = f64x2{xx[0], xx[1]};
        reinterpret_cast<f64x2 *>(ck + j)[1] = f64x2{xx[2], xx[3]};
    }, red);
}

// ------------------------------------------------------------------------------------------
// w: as k_seq_wkv reads it, with w.saa / w.sbb = this layer's aa / bb of slot 0 (read only), w.slot_stride = L D and w.ckpt_aa / w.ckpt_bb = this
// layer's checkpoint rows [T][D] (w.par, w.slot0 unused); from: [T] of the pass
struct SpecSegWkvArgs {
    SeqWkvArgs w;
    const SegRow *plan;          // [T] of the pass
    const unsigned char *from;
};
// WHERE THE STATE AFTER EACH ROW IS KEPT, AND WHERE A ROW'S START STATE COMES FROM.  The one-stream verify (k_seq_wkv<32, true>) reads the state after
// row t off the walk's own tables: the state before row t + 1 IS the state after row t.  A restart breaks that, and so does a branch.  Here the walk
// writes the state after row t into two tables of its own, aa0[t] and bbn[t], and they are its memory as well: row t starts from aa0[f] / bbn[f],
// f = from[t], and leaves its own state in aa0[t] / bbn[t]:
//   f < t    the state after row f, which the walk stored when it stepped over f -- earlier, the rows are in topological order;
//   f == t   a first row: the (row, channel) threads put the slot's aa / bb into aa0[t] / bbn[t] before the walk, and the walk reads them just before
//            it overwrites them with the state after row t.  No other row reads row t's entries in front of that point (its children lie behind it).
// One rule for every row, so the walk has NO branch: `from` stands where first flags would (one table of TCAP + 1 bytes-as-words).  Two LDS stores
// per step, nothing global on the serial thread, which reads and writes LDS only; f is the same for the 16 channels of the wave: every read is one
// broadcast-free row of 128 bytes.  The TCAP x 16 threads then store both tables to the checkpoint arrays in rows of 128 bytes.
// REGISTERS OR LDS WHERE from[t] == t - 1.  A chain carries aa / bb in registers; a read back out of LDS in every step puts a store -> load round trip into
// the one serial dependency.  Here the loads of row t + 1's start state are issued in step t, BEFORE the step's arithmetic and stores: unless
// from[t + 1] == t their source was stored in an earlier step, so they are right; where from[t + 1] == t -- every row of a chain, the first child of
// every node -- the loaded pair is stale and is dropped for the registers by two selects on a wave-uniform condition.  The results cannot depend on
// which side is taken: the tables hold exact copies of the registers.  Measured (profiles/spec_trees/wkv_kernels.txt): this form, a
// walk that reads LDS in every step behind the stores, and a walk for chains alone that never reads the tables back all take 13.3 us at 64 rows and
// 8.1 .. 8.5 us at 32 at 7B, inside what one kernel varies by between processes -- the walk is not what the kernel's time is made of.  This form was
// never the slower one and stays.
// LDS: seven [TCAP][16] f64 tables and the from table: 28 808 bytes at TCAP = 32, 57 608 (56.26 KB) at 64 (static limit 64 KB; two workgroups of 16
// waves fit a CU's 160 KB, which is what its 32 wave slots hold anyway).  A walk that stored to the checkpoint arrays itself would need six tables
// (49 KB), but puts 2 x 64 global stores with their address arithmetic into the one serial wave that everything else waits for.
template <int TCAP>
__global__ __launch_bounds__(TCAP * WKV_CH) void k_specseg_wkv(SpecSegWkvArgs g)
{
    __shared__ double e1s[TCAP][WKV_CH], eks[TCAP][WKV_CH], vs[TCAP][WKV_CH], sgs[TCAP][WKV_CH], aas[TCAP][WKV_CH], aa0[TCAP][WKV_CH], bbn[TCAP][WKV_CH];
    __shared__ unsigned froms[TCAP + 1];
    const SeqWkvArgs &a = g.w;
    RWKV_ARGS_NOW(g.plan, g.from, a.ckpt_aa, a.ckpt_bb);      // (see k_seq_resid)
    RWKV_ARGS_NOW(a.pk, a.qpart, a.uw, a.ew, a.saa, a.sbb, a.y);
    const int ch = threadIdx.x & (WKV_CH - 1), t = threadIdx.x / WKV_CH;     // t: row of the pass
    const int i = blockIdx.x * WKV_CH + ch;
    const bool live = i < a.D && t < a.T;
    if (t < a.T) {
        const SegRow row = g.plan[t];
        const bool first = seg_first(row, t);
        if (ch == 0) froms[t] = first ? (unsigned)t : min((unsigned)g.from[t], (unsigned)t);      // (the clamp: see k_specseg_site)
        if (live) {
            // a piece's start state, every first row at once, where the walk looks for ANY row's start state
            if (first) { const size_t so = (size_t)row.slot * a.slot_stride + i; aa0[t][ch] = a.saa[so]; bbn[t][ch] = a.sbb[so]; }
            seq_wkv_terms(a, t, i, e1s[t][ch], eks[t][ch], vs[t][ch], sgs[t][ch]);
        }
    }
    if (threadIdx.x == 0) froms[a.T] = 0u;      // what the last step "loads ahead": row 0, never used
    __syncthreads();
    if (threadIdx.x < WKV_CH && i < a.D) {
        const double ew = a.ew[i];
        unsigned f = froms[0];                  // (0: row 0 is a first row)
        double aa = 0.0, bb = 0.0, la = aa0[f][ch], lb = bbn[f][ch];
        for (int tt = 0; tt < a.T; tt++) {
            const bool carry = f + 1u == (unsigned)tt;       // the row in front: the registers hold its state, the loaded pair is stale
            aa = carry ? aa : la; bb = carry ? bb : lb;
            f = froms[tt + 1];
            la = aa0[f][ch]; lb = bbn[f][ch];   // row tt + 1's start state, under this step (right unless f == tt, where it is dropped above)
            seq_wkv_step(aa, bb, eks[tt][ch], vs[tt][ch], aas[tt][ch], ew);
            aa0[tt][ch] = aa; bbn[tt][ch] = bb; // the state after row tt: the checkpoint, and what the rows that name tt start from
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
// one entry per segment, uploaded with the ids and the plan or written by a lookup round kernel: the segment's last CERTAIN row r0 + c (the tree's
// root: its pick is the first one a draft id is held to), the number of draft rows behind it, the slot, and whether the segment's stream is live (a
// verify call: always 1; a lookup loop: 0 once the stream has its ids)
struct SpecSegEntry { unsigned rc, n_draft, slot, live; };
struct SpecSegRec { unsigned long long a, next, row; };      // what stands of segment i: the host's download, and what the commit reads
struct SpecSegAcceptArgs {
    const unsigned long long *ids;         // [T] the ids the pass was fed
    const unsigned long long *pick;        // [T] the picks of the rows
    const unsigned char *from;             // [T]
    const SpecSegEntry *tab;               // [n_segs]
    SpecSegRec *rec;                       // [n_segs], what k_specseg_commit reads
    unsigned long long *emitted;           // [n_segs][SPEC_MAX_DRAFT] the accepted ids in path order (the first rec.a of a row are written)
};
// One wave per segment (blockIdx.x), lane j = draft row rc + 1 + j.  conf: the id fed at the row is the pick of its parent's row.  A row STANDS when
// it and all its ancestors are confirmed: stand = conf & (the parent is the root | the parent stands), iterated from the empty set until it no longer
// grows -- round k adds the standing rows of depth k, so at most depth + 1 ballots.  Siblings carry distinct ids, so one child of a node at the most is
// confirmed and the rows that stand are ONE path from the root; in topological order the highest of them is its end, and the number of standing rows
// below lane j is j's place on the path.  On a chain the standing set is the confirmed prefix, its popcount the prefix's length a, its end row rc + a.
// A retired entry's record names no row of any pass: k_specseg_commit leaves the slot bit for bit as it stood, the next round kernel applies nothing.
template <unsigned NT> __global__ __launch_bounds__(NT) void k_specseg_accept(const SpecSegAcceptArgs g)
{
    static_assert(NT == 64 && SPEC_MAX_DRAFT < NT, "one wave, one lane per draft row");
    const SpecSegEntry e = g.tab[blockIdx.x];
    const unsigned j = threadIdx.x;
    if (!e.live) {
        if (j == 0) g.rec[blockIdx.x] = SpecSegRec{0ull, 0ull, ~0ull};
        return;
    }
    const bool draft = j < e.n_draft;
    const unsigned r = draft ? e.rc + 1u + j : e.rc;                          // (the lanes behind the tree look at the root and never stand)
    const unsigned p = draft ? min(max((unsigned)g.from[r], e.rc), r - 1u) : e.rc;      // (inside rc .. r - 1 by the host's checks)
    const unsigned long long id = g.ids[r];
    const bool conf = draft && id == g.pick[p];
    unsigned long long stand = 0ull;
    for (unsigned k = 0; k <= SPEC_MAX_DRAFT; k++) {
        const unsigned long long s = __ballot(conf && (p == e.rc || ((stand >> (p - e.rc - 1u)) & 1ull) != 0ull));
        if (s == stand) break;
        stand = s;
    }
    const unsigned acc = (unsigned)__popcll(stand);
    const unsigned row = stand ? e.rc + 64u - (unsigned)__clzll((long long)stand) : e.rc;
    if ((stand >> j) & 1ull) g.emitted[(size_t)blockIdx.x * SPEC_MAX_DRAFT + __popcll(stand & ((1ull << j) - 1ull))] = id;
    if (j == 0) g.rec[blockIdx.x] = SpecSegRec{acc, g.pick[row], row};
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
    if (row >= g.rows) return;             // (a live entry never: k_specseg_accept writes a row of the pass; a retired entry always)
    const size_t l = e / g.D, j = e - l * g.D, arr = LD * g.rows, src = (l * g.rows + (size_t)row) * g.D + j;
    const size_t dst = (size_t)g.tab[blockIdx.y].slot * LD + e;
    const f64x2 xy = *reinterpret_cast<const f64x2 *>(g.ckpt + src), aa = *reinterpret_cast<const f64x2 *>(g.ckpt + arr + src);
    const f64x2 bb = *reinterpret_cast<const f64x2 *>(g.ckpt + 2 * arr + src), dd = *reinterpret_cast<const f64x2 *>(g.ckpt + 3 * arr + src);
    *reinterpret_cast<f64x2 *>(g.xy + dst) = xy; *reinterpret_cast<f64x2 *>(g.aa + dst) = aa;
    *reinterpret_cast<f64x2 *>(g.bb + dst) = bb; *reinterpret_cast<f64x2 *>(g.dd + dst) = dd;
}

} // namespace rwkvk
