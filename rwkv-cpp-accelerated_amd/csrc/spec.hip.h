// spec.hip.h -- speculative greedy decoding ON THE DEVICE (gfx950, wave64): what stands of a draft, and the commit of exactly that row's state.
// include/rwkv_mi355x.h rwkv_spec_verify has the contract.  No reference counterpart: the reference decodes token by token.
//
// The verify pass is a GPT-mode pass of the chunk path over the rows [token, draft[0], .., draft[n - 1]] with the CKPT instances of k_seq_site
// and k_seq_wkv (seq.hip.h): it commits nothing and leaves, per layer and row, what the state holds once that row is the last one fed --
// ckpt[which][l][t][D] f64, which = 0 xy (LayerNorm output of the time-mix site), 1 aa, 2 bb (WKV state after the row), 3 dd (LayerNorm output
// of the channel-mix site).  The head runs on every row and k_argmax_rows picks every row (logit 0 banned, ties to the lowest id, no winner 0).
//     k_spec_accept   ONE wave behind the picks: a = the number of leading i with draft[i] == pick[i]; the record {a, pick[a]}.  Row a is the
//                     last row that was fed rightly: rows 0 .. a consumed token, draft[0 .. a - 1], and pick[a] is the id that follows them
//     k_spec_commit   grid over L D: reads a from the record and writes xy, aa, bb, dd of slot 0 from checkpoint row a.  pp is not touched
//                     (the chunk path does not use it)
// Both run on the pass's stream right behind it: the host learns a and the next id from one 16-byte download and waits for nothing in between.
// Plain C++ and vector memory operations only; nothing here writes host memory or waits for anything.
#pragma once
#include "seq.hip.h"

namespace rwkvk {

constexpr unsigned SPEC_MAX_DRAFT = SEQ_T - 1;       // RWKV_SPEC_MAX_DRAFT: the rows are one half of a pass
constexpr int SPEC_COMMIT_NT = 256;

struct SpecAcceptArgs {
    const unsigned long long *rows;        // [n_draft + 1] the ids the pass was fed: token, then the draft
    const unsigned long long *pick;        // [n_draft + 1] the picks of the rows
    unsigned long long *rec;               // {a, pick[a]}
    unsigned n_draft;
};
// Templates (one instance each) so that hipcc emits them where the host code first names them, behind every kernel of the decode and chunk paths
// (beam.hip.h k_beam_select has the measurement)
template <unsigned NT> __global__ __launch_bounds__(NT) void k_spec_accept(const SpecAcceptArgs a)
{
    static_assert(NT == 64 && SPEC_MAX_DRAFT < NT, "one wave, one lane per draft id");
    const unsigned i = threadIdx.x;
    const bool miss = i >= a.n_draft || a.rows[i + 1] != a.pick[i];      // (lane n_draft and the lanes behind it always miss: a <= n_draft)
    const unsigned long long m = __ballot(miss);
    const unsigned acc = (unsigned)__ffsll((long long)m) - 1u;
    if (i == acc) { a.rec[0] = acc; a.rec[1] = a.pick[acc]; }
}

struct SpecCommitArgs {
    const unsigned long long *rec;         // k_spec_accept's record
    const double *ckpt;                    // [4][L][rows][D]
    double *xy, *aa, *bb, *dd;             // slot 0 of the four state arrays, [L][D]
    unsigned L, D, rows;                   // rows of the pass = n_draft + 1
};
template <int NT> __global__ __launch_bounds__(NT) void k_spec_commit(const SpecCommitArgs a)
{
    const size_t LD = (size_t)a.L * a.D, e = (size_t)blockIdx.x * NT + threadIdx.x;
    if (e >= LD) return;
    const unsigned long long acc = a.rec[0];
    if (acc >= a.rows) return;             // (never: k_spec_accept writes a <= n_draft)
    const size_t l = e / a.D, j = e - l * a.D, arr = LD * a.rows, src = (l * a.rows + (size_t)acc) * a.D + j;
    const double xy = a.ckpt[src], aa = a.ckpt[arr + src], bb = a.ckpt[2 * arr + src], dd = a.ckpt[3 * arr + src];
    a.xy[e] = xy; a.aa[e] = aa; a.bb[e] = bb; a.dd[e] = dd;
}

} // namespace rwkvk
