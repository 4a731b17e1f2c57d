// constrain.hip.h -- constrained decoding for the device decode loops (gfx950): a token-level automaton and a sparse per-stream logit bias
// decide what a stream may generate at all; include/rwkv_mi355x.h rwkv_decode_batch_constrained has the contract, include/rwkv_sampler.h
// constrained_row / constraint_next are the same arithmetic on the host.
//
// No pick kernel knows about the constraint.  A step writes the constrained row c -- c_i = l_i + b_i where the stream's automaton state q
// has an edge on i, -inf otherwise -- into a SECOND buffer packed like the logits buffer, and the existing pick runs on that buffer; the
// model's logits are never written, so the log-prob hook and the park buffer keep seeing the model's rows.
//     k_constraint_mask     once per upload, one workgroup per state: the CSR row as a bit mask of CN_WORDS words (6288 bytes: every row is
//                           16-byte aligned); a state without edges is terminal and gets every bit but bit 0, so that a row that keeps
//                           running behind its stream's end still picks a valid id
//     k_constrain_rows      grid (CN_SLICES, rows): slice p of row r's 16-byte aligned body with 16-byte loads and stores (k_argmax_rows'
//                           split of a row: slice 0 also owns the <= 3 elements in front of the body and behind it); the workgroup that
//                           owns an id's slice applies that id's bias behind its own stores, so nothing is ordered across workgroups
//     k_constraint_advance  behind the pick and in front of k_stop_step, one thread per stream: q <- next[e] for the edge e of q on the
//                           pick (binary search), done[s] = the new state is terminal; a stream the stopper has ended is skipped, so its
//                           q freezes where it stopped.  In the one-stream greedy loop it also feeds the pick back (k_argmax_finish's part)
// Every kernel is a template (its one instance: <0>), so that hipcc emits it where the host code first names it -- behind every kernel of the
// decode and chunk paths (beam.hip.h k_beam_select has the measurement).  Plain C++ and vector memory operations only.
#pragma once
#include "kernels.hip.h"

namespace rwkvk {

constexpr unsigned CN_WORDS = (VOCAB + 31u) / 32u;     // 1572 mask words per state
static_assert(CN_WORDS == 1572u && (CN_WORDS * 4u) % 16u == 0u, "a mask row is 6288 bytes: whole 16-byte vectors");
constexpr unsigned CN_LAST = (1u << (VOCAB - (CN_WORDS - 1u) * 32u)) - 1u;     // the valid bits of the last word: ids 50272 .. 50276
static_assert(CN_LAST == 0x1Fu, "five valid bits in the last mask word");
constexpr int CN_NT = 256;                 // threads per workgroup of the mask and row kernels
constexpr int CN_SLICES = 16;              // workgroups per row of k_constrain_rows
constexpr int CN_ADV_NT = 64;              // threads per workgroup of k_constraint_advance
constexpr unsigned CN_MAX_STATES = 4096u, CN_MAX_BIAS = 300u;
constexpr unsigned CN_STOP_REASON = 32u;   // RWKV_STOP_CONSTRAINT

// the automaton in CSR form on the device: the edges of state s are row_ptr[s] .. row_ptr[s + 1], tok strictly ascending inside a row
struct CsrArgs {
    const unsigned *row_ptr;               // [S + 1]; nullptr: one state without edges (the implicit state of a call without an automaton)
    const unsigned *tok, *next;            // [nnz]
    unsigned S;
};

// grid (S): mask row s, built in LDS and written once
template <int I> __global__ __launch_bounds__(CN_NT) void k_constraint_mask(const CsrArgs a, unsigned *__restrict__ mask)
{
    __shared__ unsigned m[CN_WORDS];
    const unsigned s = blockIdx.x;
    const unsigned e0 = a.row_ptr ? a.row_ptr[s] : 0u, e1 = a.row_ptr ? a.row_ptr[s + 1] : 0u;
    const bool terminal = e0 == e1;
    for (unsigned w = threadIdx.x; w < CN_WORDS; w += CN_NT) m[w] = !terminal ? 0u : w == 0u ? ~1u : w == CN_WORDS - 1u ? CN_LAST : ~0u;
    __syncthreads();
    for (unsigned e = e0 + threadIdx.x; e < e1; e += CN_NT) {
        const unsigned t = a.tok[e];
        if (t < VOCAB) atomicOr(&m[t >> 5], 1u << (t & 31u));     // (the host has checked 1 <= t < V: the test keeps a bad upload inside the row)
    }
    __syncthreads();
    unsigned *dst = mask + (size_t)s * CN_WORDS;
    for (unsigned w = threadIdx.x; w < CN_WORDS; w += CN_NT) dst[w] = m[w];
}

struct ConstrainArgs {
    const float *logits;                   // [max_ctx][V] the model's rows: read only
    float *out;                            // [max_ctx][V] the constrained rows; same offset inside 16 bytes as `logits`
    int row;                               // row of blockIdx.y = 0 (< 0: ctl->out_row); blockIdx.y = r handles the row r behind it
    const Ctl *ctl;
    const unsigned *mask;                  // [S][CN_WORDS]
    const unsigned *q;                     // [max_ctx] the slots' automaton states; nullptr: mask row 0 for every row
    unsigned slot;                         // slot of blockIdx.y = 0
    const unsigned *bias_ptr;              // [rows + 1] stream r's pairs are bias_ptr[r] .. bias_ptr[r + 1]; nullptr: no bias
    const unsigned *bias_tok;              // ascending inside a stream, 1 .. V - 1
    const float *bias_val;                 // finite or -inf
};

__device__ __forceinline__ bool cn_bit(const unsigned *__restrict__ mrow, unsigned i) { return (mrow[i >> 5] >> (i & 31u)) & 1u; }

template <int I> __global__ __launch_bounds__(CN_NT) void k_constrain_rows(const ConstrainArgs a)
{
    const int V = (int)VOCAB;
    const size_t r = (size_t)(a.row >= 0 ? (unsigned)a.row : a.ctl->out_row) + blockIdx.y;
    const float *lg = a.logits + r * V;
    float *dst = a.out + r * V;
    const unsigned state = a.q ? a.q[a.slot + blockIdx.y] : 0u;
    const unsigned *mrow = a.mask + (size_t)state * CN_WORDS;
    const int h = (int)(((16u - ((unsigned)(uintptr_t)lg & 15u)) & 15u) >> 2);   // elements in front of the first 16-byte boundary (dst: the same)
    const int nv = (V - h) >> 2;                                                  // float4s of the aligned body
    const f32x4 *body = reinterpret_cast<const f32x4 *>(lg + h);
    f32x4 *obody = reinterpret_cast<f32x4 *>(dst + h);
    const int v0 = block_lo(nv), v1 = block_hi(nv);
#pragma unroll 4
    for (int v = v0 + (int)threadIdx.x; v < v1; v += CN_NT) {
        const f32x4 x = body[v];
        const unsigned i = (unsigned)(h + 4 * v);                                 // i + 3 < V: the words read lie inside the mask row
        const unsigned w0 = mrow[i >> 5], w1 = mrow[(i + 3u) >> 5];
        f32x4 c;
#pragma unroll
        for (unsigned k = 0; k < 4u; k++) {
            const unsigned j = i + k;
            const unsigned w = (j >> 5) == (i >> 5) ? w0 : w1;
            c[k] = ((w >> (j & 31u)) & 1u) ? x[k] + 0.0f : -INFINITY;             // b_i = 0 where i is not listed: the one f32 add all the same
        }
        obody[v] = c;
    }
    if (blockIdx.x == 0 && threadIdx.x < 8) {      // head [0, h) on threads 0..3, tail [h + 4 nv, V) on threads 4..7
        const int i = threadIdx.x < 4 ? (int)threadIdx.x : h + 4 * nv + (int)threadIdx.x - 4;
        if (i < (threadIdx.x < 4 ? h : V)) dst[i] = cn_bit(mrow, (unsigned)i) ? lg[i] + 0.0f : -INFINITY;
    }
    if (!a.bias_ptr) return;
    __syncthreads();                               // this workgroup's stores are ordered in front of its bias stores
    const unsigned b0 = a.bias_ptr[blockIdx.y], b1 = a.bias_ptr[blockIdx.y + 1];
    const int lo = h + 4 * v0, hi = h + 4 * v1;    // the body elements this workgroup owns
    for (unsigned b = b0 + threadIdx.x; b < b1; b += CN_NT) {
        const int i = (int)a.bias_tok[b];
        if (i <= 0 || i >= V) continue;            // (checked on the host)
        const bool mine = (i >= lo && i < hi) || (blockIdx.x == 0 && (i < h || i >= h + 4 * nv));
        if (mine && cn_bit(mrow, (unsigned)i)) dst[i] = __fadd_rn(lg[i], a.bias_val[b]);
    }
}

struct AdvanceArgs {
    CsrArgs csr;                           // S == 0: no automaton -- nothing to advance, only the feedback
    unsigned *q;                           // [max_ctx]
    unsigned slot;                         // slot of stream 0
    unsigned n;                            // streams
    unsigned *done;                        // [n] 1 when the state reached at this step is terminal, else 0; nullptr: not recorded
    const unsigned *len;                   // [n] the stopper's lengths: a stream with len != 0 has ended and is skipped; nullptr: none has
    int feedback;                          // one-stream greedy loop: the pick goes into ctl->token and gen[ctl->step], the step advances
    Ctl *ctl;
    unsigned long long *gen;
    unsigned gen_cap;
};

// picks: [n] the ids picked at this step
template <int I> __global__ __launch_bounds__(CN_ADV_NT) void k_constraint_advance(const AdvanceArgs a, const unsigned long long *__restrict__ picks)
{
    const unsigned s = blockIdx.x * CN_ADV_NT + threadIdx.x;
    if (s >= a.n) return;
    const unsigned g = (unsigned)picks[s];
    if (a.feedback && s == 0) {
        const unsigned st = a.ctl->step;
        if (st < a.gen_cap) a.gen[st] = g;
        a.ctl->token = g;
        a.ctl->step = st + 1;
    }
    if (a.len && a.len[s]) return;
    unsigned fin = 0u;
    if (a.csr.S) {
        const unsigned cur = a.q[a.slot + s];
        unsigned lo = a.csr.row_ptr[cur], hi = a.csr.row_ptr[cur + 1];
        while (lo < hi) {                  // the first edge with tok >= g
            const unsigned mid = lo + ((hi - lo) >> 1);
            if (a.csr.tok[mid] < g) lo = mid + 1; else hi = mid;
        }
        if (lo < a.csr.row_ptr[cur + 1] && a.csr.tok[lo] == g) {
            const unsigned nx = a.csr.next[lo];
            if (nx < a.csr.S) {            // (checked on the host)
                a.q[a.slot + s] = nx;
                fin = a.csr.row_ptr[nx] == a.csr.row_ptr[nx + 1] ? 1u : 0u;
            }
        }                                  // no edge on the pick (logits that are no numbers): the state stays
    }
    if (a.done) a.done[s] = fin;
}

} // namespace rwkvk
