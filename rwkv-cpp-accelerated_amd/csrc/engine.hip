// engine.hip -- host runtime + C-ABI of librwkv_mi355x.so (see include/rwkv_mi355x.h).
//
// Replaces the reference's backend translation unit include/rwkv/cuda/rwkv.cu (load / setState /
// getOutput / freeTensors / cuda_rwkv_parralel, declared rwkv.h:63-122) with an opaque-handle
// engine: weights are re-tiled once at load, state and the embedding table stay resident on the
// device, and one token is a replay of a captured hipGraph (4 launches per layer + 2).
#include "kernels.hip.h"
#include "tile.hip.h"
#include "seq.hip.h"
#include "sampler.hip.h"
#include "nucleus.hip.h"
#include "score.hip.h"
#include "topn.hip.h"
#include "stop.hip.h"
#include "beam.hip.h"
#include "constrain.hip.h"
#include "spec.hip.h"
#include "segments.hip.h"
#include "../../include/rwkv_mi355x.h"
#include "../../include/rwkv_sampler.h"

#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <unistd.h>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

using namespace rwkvk;

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e__ = (expr);                                                                       \
        if (e__ != hipSuccess)                                                                         \
            return fail(RWKV_E_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)

// tensor slots of model.bin, reference enums/enum.h:7-55
enum {
    X, EMBED, LAYERNORMS, STATEXY, STATEAA, STATEBB, STATEPP, STATEDD, BUFFER1, BUFFER2, BUFFER3, BUFFER4,
    MIXK, MIXV, MIXR, KM, VM, RM, KR, VR, RR, O1, O2, O3, ATTOUT, ATTOUTR, ATTOUTO, FFNMIXK, FFNMIXV,
    FFNK, FFNV, FFNR, FFNKR, FFNVR, FFNRR, FFNKO, FFNVO, FFNRO, FFNKBUFFER, FFNVBUFFER, FFNRBUFFER,
    DECAY, BONUS, HEAD, HEADR, HEADO
};
// element sizes / counts: reference rwkv.h:84 and rwkv.h:124-128
const uint64_t kTypes[46] = {8, 4, 8, 8, 8, 8, 8, 8, 8, 4, 4, 4, 8, 8, 8, 1, 1, 1, 4, 4, 4, 4, 4,
                             4, 1, 4, 4, 8, 8, 1, 1, 1, 4, 4, 4, 4, 4, 4, 8, 8, 4, 8, 8, 1, 4, 4};
uint64_t tensor_elems(int i, uint64_t a, uint64_t b)
{
    const uint64_t V = RWKV_VOCAB;
    const uint64_t s[46] = {b, V * b, 4 * (a + 1) * b, a * b, a * b, a * b, a * b, a * b, b, V, b, b,
                            a * b, a * b, a * b, a * b * b, a * b * b, a * b * b, a * b, a * b, a * b, a * b, a * b, a * b,
                            a * b * b, a * b, a * b, a * b, a * b, a * b * b * 4, a * b * b * 4, a * b * b,
                            a * b, a * b * 4, a * b, a * b, a * b * 4, a * b, b, b, b * 4, a * b, a * b, V * b, b, b};
    return s[i];
}

// where tensor bytes come from during a load, and how they reach the device.  A model.bin (8 GB at 7B) streams through
// two pinned staging buffers: the file read of piece i + 1 overlaps the host-to-device copy of piece i, nothing waits for
// the device until the load is complete (round 1 read every tensor into a pageable buffer and synchronised per tensor).
struct Source {
    FILE *f = nullptr;                  // model.bin, or
    const void *const *ptrs = nullptr;  // 46 pointers in file layout
    bool on_device = false;
    uint64_t off[46];
    static constexpr size_t PIN = 32u << 20;
    unsigned char *pin[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool used[2] = {false, false};
    int turn = 0;
    // device pointer of a tensor that already lives on the device (on_device sources), else nullptr
    const void *device_ptr(int i, uint64_t o) const { return (ptrs && on_device && ptrs[i]) ? static_cast<const unsigned char *>(ptrs[i]) + o : nullptr; }
    // enqueue bytes [o, o + n) of tensor i -> dst (device) on `stream`; the caller's later work on the stream sees them
    int to_device(int i, uint64_t o, uint64_t n, void *dst, hipStream_t stream)
    {
        if (ptrs) {
            if (!ptrs[i]) return fail(RWKV_E_IO, "tensor slot %d: missing", i);
            // caller-owned memory stays valid for the whole load: no staging, no wait
            HIPCHK(hipMemcpyAsync(dst, static_cast<const unsigned char *>(ptrs[i]) + o, n, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
            return 0;
        }
        if (fseeko(f, (off_t)(off[i] + o), SEEK_SET) != 0) return fail(RWKV_E_IO, "tensor slot %d: seek failed", i);
        for (uint64_t done = 0; done < n;) {
            const size_t m = (size_t)std::min<uint64_t>(PIN, n - done);
            const int b = turn;
            turn ^= 1;
            if (!pin[b]) {
                HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&pin[b]), PIN, hipHostMallocDefault));
                HIPCHK(hipEventCreateWithFlags(&ev[b], hipEventDisableTiming));
            }
            if (used[b]) HIPCHK(hipEventSynchronize(ev[b]));          // the copy that last read this buffer has finished
            if (fread(pin[b], 1, m, f) != m) return fail(RWKV_E_IO, "tensor slot %d: short read", i);
            HIPCHK(hipMemcpyAsync(static_cast<unsigned char *>(dst) + done, pin[b], m, hipMemcpyHostToDevice, stream));
            HIPCHK(hipEventRecord(ev[b], stream));
            used[b] = true;
            done += m;
        }
        return 0;
    }
    ~Source()
    {
        for (int b = 0; b < 2; b++) {
            if (used[b]) (void)hipEventSynchronize(ev[b]);
            if (ev[b]) (void)hipEventDestroy(ev[b]);
            if (pin[b]) (void)hipHostFree(pin[b]);
        }
    }
};

} // namespace

// RCCL (librccl.so, resolved at run time by rwkv_pipe_init: a single-GPU user never loads it) -- the subset of rccl.h the
// layer pipeline needs.  Types per /opt/rocm/include/rccl/rccl.h (ncclUniqueId = 128 opaque bytes; ncclUint64 = 5, ncclFloat64 = 8).
struct Pipe {
    void *lib = nullptr;
    void *comm = nullptr;
    int rank = 0, world = 1;
    struct Id { char b[128]; };
    int (*GetUniqueId)(Id *) = nullptr;
    int (*CommInitRank)(void **, int, Id, int) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*Send)(const void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*Recv)(void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    int (*GetVersion)(int *) = nullptr;
    // two-communicator schedule (rwkv_pipe_decode_dual): sub-schedule k = streams of parity k on comm k (comm / comm2) and HIP stream cs[k],
    // hop buffers per parity, events between the comm streams and the engine's compute stream
    void *comm2 = nullptr;
    hipStream_t cs[2] = {nullptr, nullptr};
    double *xin[2] = {nullptr, nullptr}, *xout[2] = {nullptr, nullptr};
    unsigned long long *idbuf[2] = {nullptr, nullptr};
    hipEvent_t ev_rx[2] = {nullptr, nullptr}, ev_cp[2] = {nullptr, nullptr};
    bool dual_ready = false;     // every resource of the two-communicator schedule AND comm2 exist (pipe_dual_setup)
    uint64_t ch = 0;             // rows per prefill micro-batch every rank of this pipeline agreed on (rwkv_pipe_init)
    std::string info;            // one JSON object describing this rank's end of the transport (rwkv_pipe_info)
};

// per-chunk scratch of the chunk path (one set per pipeline stage that may be in flight).  Everything per chunk is sized for a pass of
// SEQ_TM = 64 rows = two halves: half 1's images / records / partial values sit right behind half 0's (seq.hip.h SEQ_TM)
struct SeqScratch {
    double *state = nullptr;            // [D] LayerNorm output of the chunk's last token
    float *y = nullptr;                 // gated wkv output [SEQ_TM][D]
    unsigned *img[3] = {nullptr, nullptr, nullptr}, *imgh = nullptr;   // MFMA A-operand images (K = D; K = 4D)
    SeqPart *qpart = nullptr, *qparta = nullptr, *qparth = nullptr;    // quantisation records: site vectors [3][SEQ_T][SEQ_O], att_out input [SEQ_T][SEQ_O], ffn_v input [SEQ_T][SEQ_O]
    SeqStat *stat = nullptr;            // [SEQ_TM][SEQ_O] LayerNorm partial statistics
    float *pk3 = nullptr, *pk5 = nullptr, *pk1 = nullptr;   // per-slice partial values of the K/V/R, ffn k/r, att_out | ffn_v GEMMs (accumulator images, seq.hip.h pk_index)
    double *seg = nullptr;              // segmented passes only (allocated at the first one that uses the set): [SEQ_TM][D] LayerNorm outputs of the pieces' last rows
};
// Elements of ONE half of a scratch set at width D: the allocation holds two of each, and a pass of two halves finds half 1 at these offsets
struct SeqHalf {
    size_t img, imgh;                   // A-image 32-bit words for K = D and K = 4 D
    size_t part3, part1;                // records of a 3-vector and a 1-vector site
    size_t pk3, pk5, pk1;               // partial values [slice][tile][2][4][64] of 3, 5 and 1 row classes, tiles = classes x 16-channel blocks
    explicit SeqHalf(size_t D)
        : img(a_image_bytes(D) / 4), imgh(a_image_bytes(4 * D) / 4), part3((size_t)3 * SEQ_T * SEQ_O), part1((size_t)SEQ_T * SEQ_O),
          pk3((size_t)SEQ_O * 3 * ((D + 15) / 16) * 512), pk5((size_t)SEQ_O * 5 * ((D + 15) / 16) * 512), pk1((size_t)SEQ_O * ((D + 15) / 16) * 512) {}
};
// One GEMM of the chunk path as a context launches it: everything that follows from the width, RWKV_SEQ_B, the GEMM's kind (0 K/V/R, 1 att_out,
// 2 ffn k/r, 3 ffn_v) and whether the pass has one or two halves -- and not from the pass.  seq_gemm_plan() fills it, load_common keeps the table.
//   args          the argument block but for what a pass and a layer set (enqueue_chunk's gemm); k_seq_gemm_p takes args.g
//   fn_p | fn_b   the form and its instance: k_seq_gemm_p or k_seq_gemm_b (the other is null)
//   smem          the instance's LDS bytes (k_seq_gemm_b: of its longest slice; a launch asks for its own, nkb_max k-blocks)
//   grid          workgroups
struct SeqGemmPlan { SeqGemmBArgs args{}; void (*fn_p)(SeqGemmArgs) = nullptr; void (*fn_b)(SeqGemmBArgs) = nullptr; size_t smem = 0; int grid = 0, nkb_max = 0; };

// One weight class: the uint8 matrices one decode kernel streams and one GEMM of the chunk path multiplies with.  N = Q row classes x `rows`
// outputs (rows = D, or the vocabulary for the head), K = kd D inputs.  What a layer of it occupies follows from those three; which tensors of the
// file make its row form -- row q + RS j of the class's matrix = row j of the tensor's matrix -- is the `src` list (k_retile's arguments).
struct WSrc { int slot, n, m, G, RS, off; };     // file tensor [n D][m D] (m = 0: [D][vocabulary]), re-tiled with (G, RS, off)
struct WClass {
    int Q, kd;
    bool vocab;
    int nsrc;
    WSrc src[3];
    // device, [layers of the stage] each (the head: one): row form (nullptr: the class runs in tile form) and its row sums; the chunk
    // path's image of 16-row tiles and the row sums per octant of K; the image the tile-form decode kernel streams (= b where its tiles are 16 rows)
    uint8_t *w = nullptr, *b = nullptr, *t = nullptr;
    unsigned *rs = nullptr, *r8 = nullptr;
    uint64_t rows(uint64_t D) const { return vocab ? (uint64_t)RWKV_VOCAB : D; }
    uint64_t N(uint64_t D) const { return Q * rows(D); }
    uint64_t K(uint64_t D) const { return kd * D; }
    // per layer: bytes of the row form (and of an image of 4-row tiles: D is a multiple of 16), bytes of the 16-row image, row sums, octant row sums
    uint64_t row_bytes(uint64_t D) const { return N(D) * K(D); }
    uint64_t img_bytes(uint64_t D) const { return Q * ((rows(D) + 15) / 16) * 16 * K(D); }
    uint64_t sums(uint64_t D) const { return N(D); }
    uint64_t sums8(uint64_t D) const { return SEQ_O * N(D); }
    // layer wl of the stage
    const uint8_t *w_at(uint64_t wl, uint64_t D) const { return w ? w + wl * row_bytes(D) : nullptr; }
    const uint8_t *b_at(uint64_t wl, uint64_t D) const { return b + wl * img_bytes(D); }
    const uint8_t *t_at(uint64_t wl, uint64_t D) const { return t + wl * row_bytes(D); }      // (a layer's images are as large as its row form: D is a multiple of 16)
    const unsigned *rs_at(uint64_t wl, uint64_t D) const { return rs + wl * sums(D); }
    const unsigned *r8_at(uint64_t wl, uint64_t D) const { return r8 + wl * sums8(D); }
};

// The device buffers of batched decode (rwkv_decode_batch_*) and scoring (rwkv_score_rows / rwkv_score, score.hip.h) that belong to the context:
// allocated at the first call, grown to the largest one seen (grow_buffer), freed by rwkv_free
enum GrownBuf {
    BD_IDS,                           // u64 [n seeds][n_steps + 1][n]: row 0 = the first tokens, row k + 1 = the picks of step k
    BD_VAL, BD_IDX,                   // greedy partials [n][AM_SLICES] (k_argmax_rows)
    BD_PART, BD_P, BD_PW, BD_KEY,     // sampler scratch per row [n][...] (sampler.hip.h)
    SC_IN,                            // u64 [2][n]: rows | targets; behind them the control blocks of rwkv_score's token-by-token pieces
    SC_PART,                          // f64 [queries of one launch sequence][SC_G][4] per-workgroup tuples
    SC_OUT,                           // [3][n]: logprob f64 | entropy f64 | argmax u64
    PEN_COUNTS,                       // f32 [max_ctx][V]: occurrence counts per state slot (nucleus.hip.h); allocated ONCE, zeroed, at the first call that needs them
    STOP_RUN,                         // rwkv_decode_batch_until (stop.hip.h): u64 active | u64 first [n] | u32 len [n] | u32 reason [n] | u32 max_new [n]
    STOP_PARK,                        // f32 [n][5 x 2 L D + PARK_ROW (+ PARK_ROW with penalties)]: what the streams held when they stopped
    STOP_HISTORY,                     // u32 [max_ctx][STOP_HIST]: the newest ids per state slot; allocated ONCE, emptied, at the first call that can stop a stream
    LP_REC,                           // rwkv_topn_rows / rwkv_decode_batch_logprobs (topn.hip.h), 8-byte words (LpLayout): rows [R] | score tuples [R][SC_G][4] |
                                      // candidates [R][SC_G][n] | per step: logprob [R] | entropy [R] | top ids [R][n] | top logprob [R][n]
    BEAM_REC,                         // rwkv_decode_beam / rwkv_debug_beam_step (beam.hip.h), 8-byte words (BeamLayout): ids [2][W] | stop ids [16] | cum [W] |
                                      // ended, len u32 [2][W] | parent map u32 [W] + padding | per step: parent, token u32 [2][W] | score [W] | token log-prob [W];
                                      // rwkv_state_permute: the parent map u32 [n]
    BEAM_STAGE,                       // f64 [n][5][L D]: where the state gather sets the parents' slots aside
    CN_CSR,                           // constrained decoding (constrain.hip.h), u32: row_ptr [S + 1] | tok [nnz] | next [nnz] of the installed automaton
    CN_MASK,                          // u32 [S][CN_WORDS]: the automaton's states as bit masks over the vocabulary
    CN_MASK1,                         // u32 [CN_WORDS]: the implicit state of a constrained call without an automaton (every id but 0)
    CN_ROWS,                          // f32 [max_ctx][V]: the constrained rows, packed like the logits buffer; allocated ONCE by the first call that needs it
    CN_Q,                             // u32 [max_ctx]: the slots' automaton states (cn_q is the host copy); allocated ONCE, zeroed
    CN_CALL,                          // u32, one call's upload: bias_ptr [n + 1] | bias tok [nb] | bias val f32 [nb]; behind it done [n]
    SPEC_CKPT,                        // rwkv_spec_verify (spec.hip.h): f64 [4][L][rows][D], the verify pass's checkpoints (xy | aa | bb | dd) for the largest n_draft seen
    SPEC_REC,                         // u64: {a, next} | picks [SEQ_T]
    SEG_PLAN,                         // rwkv_forward_segments (segments.hip.h): SegRow [max_ctx], the call's row plan; allocated ONCE at the first segmented call
    N_GROWN
};

struct rwkv_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int grid = 256;          // workgroups per launch = compute units
    bool loaded = false;
    uint64_t L = 0, D = 0, maxT = 1;
    uint64_t l0 = 0, l1 = UINT64_MAX;   // pipeline stage: this context owns layers [l0, l1) (whole model by default)
    int S = 0;               // ceil(D / 1024): 1 KiB row pieces per lane
    int seq_rows = SEQ_TM;   // chunk path: rows per weight pass, 64 (two halves, round 4) or 32 (env RWKV_SEQ_ROWS)
    int seq_b = -1;          // 64-row passes: GEMM kinds (bit 0 K/V/R, bit 2 ffn k/r) that run as k_seq_gemm_b -- one vector's image of the whole slice resident,
                             // a wave's tiles in batches, one round of workgroups (env RWKV_SEQ_B; 0: k_seq_gemm_p<.., true, 2>; -1: ffn k/r always, K/V/R at D >= 4096:
                             // +1-2 % there, -1.5 % at D = 2048, profiles/r04/gemm_b_ab2.txt)
    int tile = -1;           // decode kernel classes that run in TILE form (tile.hip.h; bit 0 k_att, 1 k_attout, 2 k_ffn_rk, 3 k_ffnv; env RWKV_TILE; -1 = auto: 15 at
                             // D = 4096 and 5120 on 256 CUs, 13 at D = 2048, else 0).  15: the context holds ONLY the tile image of the per-layer
                             // matrices; a partial mask keeps both layouts (tuning)

    // weights (device)
    float *embed = nullptr;
    double *ln = nullptr, *mixk = nullptr, *mixv = nullptr, *mixr = nullptr, *fmixk = nullptr, *fmixr = nullptr;
    float *kr = nullptr, *vr = nullptr, *rr = nullptr, *o1 = nullptr, *o2 = nullptr, *o3 = nullptr;
    float *attr = nullptr, *atto = nullptr, *fkr = nullptr, *fvr = nullptr, *frr = nullptr;
    float *fko = nullptr, *fvo = nullptr, *fro = nullptr, *headr = nullptr, *heado = nullptr;
    double *uw = nullptr, *ew = nullptr;
    // LayerNorm-site tables (kernels.hip.h "LayerNorm sites"): k = 0 ln1 -> K/V/R (3 vectors), 1 ln2 -> ffn k/r (2), 2 ln_out -> head (1)
    float *siteC[3] = {nullptr, nullptr, nullptr};    // [L or 1][NV][D]
    float *siteP[3] = {nullptr, nullptr, nullptr};    // [L or 1][D][PW]
    double *siteTC[3] = {nullptr, nullptr, nullptr};  // [L or 1][NV]
    float *siteMC[3] = {nullptr, nullptr, nullptr};   // [L or 1][NV]
    float *siteB[3] = {nullptr, nullptr, nullptr};    // [NV][D]   per-token, emitted by the row owners
    double *sitePD[3] = {nullptr, nullptr, nullptr};  // [grid][8] per-workgroup partial tuples
    float *sitePF[3] = {nullptr, nullptr, nullptr};   // [grid][4]
    double *lnstat = nullptr;                         // [3][2] mean, rstd per site
    // the matrices: index = decode kernel class - 1 (0 K/V/R, 1 att_out, 2 ffn k/r, 3 ffn_v), 4 = the head
    WClass wc[5] = {
        {3, 1, false, 3, {{KM, 1, 1, 1, 3, 0}, {VM, 1, 1, 1, 3, 1}, {RM, 1, 1, 1, 3, 2}}},
        {1, 1, false, 1, {{ATTOUT, 1, 1, 1, 1, 0}}},
        {5, 1, false, 2, {{FFNK, 1, 4, 4, 5, 0}, {FFNR, 1, 1, 1, 5, 4}}},      // rows 5 i + q = ffn_k output 4 i + q, row 5 i + 4 = ffn_r output i
        {1, 4, false, 1, {{FFNV, 4, 1, 1, 1, 0}}},
        {1, 1, true, 1, {{HEAD, 1, 0, 1, 1, 0}}},
    };
    // state + scratch (device)
    double *state[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    double *x = nullptr, *partA = nullptr, *partF = nullptr;
    float *ybuf = nullptr, *hbuf = nullptr, *rgate = nullptr, *logits = nullptr, *blk_val = nullptr, *partMA = nullptr, *partMF = nullptr;
    unsigned *blk_idx = nullptr;
    Ctl *ctl = nullptr;
    Ctl *h_ctl = nullptr;    // pinned staging, maxT entries
    SegRow *h_seg_plan = nullptr;   // pinned [maxT]: what rwkv_forward_segments uploads into SEG_PLAN (allocated with it)
    unsigned long long *gen = nullptr;
    unsigned long long *pick = nullptr;      // device: id drawn by the sampler
    double *ts_part = nullptr;               // sampler scratch (sampler.hip.h)
    float *ts_p = nullptr, *ts_pw = nullptr;
    unsigned *ts_key = nullptr;
    unsigned gen_cap = 0;
    hipGraphExec_t g_fwd = nullptr, g_greedy = nullptr;
    // device error word: a mapped pinned word that a kernel raises when one of its bounded waits gave up (tile-form LDS hand-offs);
    // checked after every stream synchronisation (device_check)
    unsigned *herr = nullptr, *d_herr = nullptr;
    unsigned long long *tl = nullptr;   // phase-timeline buffer (debug), [grid][NW][8]
    bool tl_on = false;
    int tl_cls = 3;                     // kernel class the timeline instruments (env RWKV_TL_CLASS, 1..4)
    // chunked (prompt prefill) path, seq.hip.h: allocated when max_ctx > 1 on a whole-model context
    bool seq_ok = false;
    SeqGemmPlan seq_plan[8];                      // [4 (halves of the pass - 1) + kind]: how this context launches each GEMM (fixed at load)
    unsigned long long *sq_tokens = nullptr;      // device, [SEQ_TM] per RESIDUAL BUFFER (token_slot): the ids of the pass in sq_x[b], what its k_seq_embed reads
                                                  // (allocated as [SQ_RING][SEQ_TM], of which slots 0 .. SPLIT_MAX - 1 are used)
    unsigned long long *h_sq_tokens = nullptr;    // pinned [SQ_RING][SEQ_TM]: the ring of staging slots the ids are uploaded from
    hipEvent_t sq_ev[8] = {};                     // slot r of the ring is free once sq_ev[r] has completed
    uint64_t sq_n = 0;                            // chunks enqueued so far
    // captured passes of the chunk path (GPT mode): one hipGraph per (layer range, residual buffer, rows, logits row of the last part);
    // a pass is 11 launches per layer -- 2.9 k launches and events for a 512-token 7B prompt, 3.5 us of host time each
    // (RWKV_GRAPH bit 1 clear: direct launches)
    struct SeqGraphKey { uint64_t la, lb, row0; int buf, n; bool operator<(const SeqGraphKey &o) const { return std::tie(la, lb, row0, buf, n) < std::tie(o.la, o.lb, o.row0, o.buf, o.n); } };
    std::map<SeqGraphKey, hipGraphExec_t> sq_graphs;
    bool seq_graph = true;
    int graphs = 3;                               // env RWKV_GRAPH: bit 0 = a decode token is a hipGraph replay, bit 1 = so is a GPT-mode pass of the chunk path (0: direct launches)
    static constexpr int SPLIT_MAX = 4;                       // stages of the one-GPU pipeline at most, and residual buffers: a chunk in flight per stage
    double *sq_x[SPLIT_MAX] = {nullptr, nullptr, nullptr, nullptr};   // residual stream [SEQ_TM][D]; two buffers: a pipeline stage receives chunk c + 1 while chunk c is sent on; [2], [3]: more chunks in flight in rwkv_forward's pipeline
    hipEvent_t xs_ev[2] = {nullptr, nullptr};     // rwkv_xseq_copy: "source chunk done" / "copied"
    // long prompts on one GPU: the chunk path as a two-stage software pipeline (layers [l0, mid) on `stream`, [mid, l1) + head on
    // `stream2`, stage 2 on chunk c while stage 1 is on chunk c + 1); the second stage has its own scratch set
    int n_split = 0;                                          // stages in use (0: not set up)
    hipStream_t sp_stream[SPLIT_MAX] = {};                    // [0] = stream (load_common)
    SeqScratch sp_scratch[SPLIT_MAX];                         // [0] = the context's own set (load_common), the others at first use (split_setup)
    hipEvent_t sp_done[SPLIT_MAX][SPLIT_MAX] = {};            // [stage][buffer]: the stage has finished the chunk in that buffer
    hipEvent_t sp_end = nullptr;
    double *x_in = nullptr;                       // decode: residual vector received from the previous stage (nullptr: c->x)
    struct Pipe *pipe = nullptr;                  // RCCL transport of the layer pipeline (rwkv_pipe_init)
    bool pipe_prof = false;                       // rwkv_pipe_profile: bracket the ticks' RCCL groups with event pairs
    static constexpr size_t HOP_EV = 512;
    hipEvent_t hop_ev[2 * HOP_EV] = {};
    double hop_stats[4] = {0.0, 0.0, 0.0, 0.0};
    Ctl *pipe_ring = nullptr;                     // pinned control blocks of rwkv_pipe_decode's items (grown on demand, kept)
    uint64_t pipe_ring_cap = 0;
    // tile-form decode kernels (tile.hip.h): they stream the chunk path's own image (16-row tiles) where a workgroup owns one 16-channel block,
    // else a decode-only image of 4-row tiles (WClass::t)
    int tile_th = 0, tile_s = 0, tile_tpc = 0;     // rows per tile, KiB per ring unit, tiles per row class and workgroup (0: no tile form at this width)
    struct Grown { void *p = nullptr; size_t bytes = 0; } grown[N_GROWN];      // (enum GrownBuf)
    template <class T> T *buf(GrownBuf which) const { return static_cast<T *>(grown[which].p); }
    std::vector<unsigned long long> bd_host, sc_host, lp_host, beam_host;   // staging of a call's one upload and one download
    static constexpr int STOP_RING = 4;           // rwkv_decode_batch_until: block b's count of active streams lands in word b % 4, read when block b + 2 is due
    unsigned long long *stop_ring = nullptr;      // pinned
    hipEvent_t stop_ev[STOP_RING] = {};
    std::vector<unsigned> stop_host;              // host image of STOP_RUN: the call's upload, and the download of lengths and reasons
    // constrained decoding: the installed automaton's size and host copy of row_ptr (cn_S == 0: none), the host copy of the slots' states
    // (kept equal to CN_Q by every call that writes it: checks need no launch) and the staging of a call's upload
    unsigned cn_S = 0;
    size_t cn_nnz = 0;
    std::vector<unsigned> cn_row_ptr, cn_q, cn_host;
    std::vector<void *> allocs;
    size_t alloc_bytes = 0;                       // device bytes behind `allocs` and the Grown buffers (rwkv_resident_bytes)
};

namespace {

template <typename T> int dalloc(rwkv_ctx *c, T **p, size_t count)
{
    void *q = nullptr;
    HIPCHK(hipMalloc(&q, std::max<size_t>(count * sizeof(T), 16)));
    c->allocs.push_back(q);
    c->alloc_bytes += std::max<size_t>(count * sizeof(T), 16);
    *p = static_cast<T *>(q);
    return 0;
}

// tile-form decode kernels (tile.hip.h; classes 1 att, 2 att_out, 3 ffn_rk, 4 ffn_v): ring of S KiB units behind each kernel's fixed LDS.
// Which widths have a tile form: those whose channels split into whole TH-row tiles per workgroup on this grid.  The three instances, each
// written once -- width, KiB per ring unit, rows per tile, tiles per row class and workgroup; the kernels' other template arguments follow:
//   D = 4096 on 256 CUs: 16 channels = ONE 16-row tile per class (the chunk path's own image; the default there)
//   D = 5120 on 256 CUs: 20 channels = five 4-row tiles (a decode-only image of 4-row tiles)
//   D = 2048 on 256 CUs:  8 channels = two 4-row tiles
template <int D_, int S_, int TH_, int TPC_> struct TileInst {
    static constexpr int D = D_, S = S_, TH = TH_, TPC = TPC_, SD = D / 1024;
    static constexpr int KBT = D * TH / 1024, KBT_FV = 4 * KBT;      // fragments (1 KiB) of a tile along K = D, and along ffn_v's K = 4 D
    static_assert(TH * TPC * 256 == D, "a workgroup's tiles are its share of the channels on 256 workgroups");
};
using Tile4096 = TileInst<4096, 4, 16, 1>;
using Tile5120 = TileInst<5120, 5, 4, 5>;
using Tile2048 = TileInst<2048, 4, 4, 2>;
struct TileCfg { int th, s, tpc; };
template <class T> TileCfg tile_cfg_of() { return TileCfg{T::TH, T::S, T::TPC}; }
TileCfg tile_cfg_for(uint64_t D, int grid)
{
    if (grid != 256) return TileCfg{0, 0, 0};
    if (D == Tile4096::D) return tile_cfg_of<Tile4096>();
    if (D == Tile5120::D) return tile_cfg_of<Tile5120>();
    if (D == Tile2048::D) return tile_cfg_of<Tile2048>();
    return TileCfg{0, 0, 0};
}
// fixed LDS bytes, ring units and launch bytes of a class, from the kernels' own description of their LDS (tile.hip.h tile_lds_of)
size_t tile_fixed(const rwkv_ctx *c, int cls) { return tile_lds_of(cls, (int)c->D, c->tile_th * c->tile_tpc).ring; }
int tile_units(const rwkv_ctx *c, int cls)
{
    const int kbt = (int)((cls == 4 ? 4 * c->D : c->D) * c->tile_th / 1024);                         // fragments of a tile along K
    return tile_ring_units(tile_fixed(c, cls), c->tile_s, tile_nu(cls, c->tile_tpc, kbt, c->tile_s));
}
size_t tile_smem(const rwkv_ctx *c, int cls) { return tile_fixed(c, cls) + (size_t)tile_units(c, cls) * c->tile_s * 1024; }
// a class runs in tile form when asked to (RWKV_TILE bit cls - 1) and its image is there
bool tile_ok(const rwkv_ctx *c, int cls)
{
    return c->tile > 0 && ((c->tile >> (cls - 1)) & 1) && c->wc[cls - 1].t != nullptr;
}
// f(the context's tile instance); f(1 .. 5 as a type): how a run-time configuration becomes template arguments
template <class F> auto by_tile(const rwkv_ctx *c, F f)
{
    if (c->tile_th == Tile4096::TH) return f(Tile4096{});
    if (c->tile_tpc == Tile5120::TPC) return f(Tile5120{});
    return f(Tile2048{});
}
template <int S> using SConst = std::integral_constant<int, S>;
template <class F> auto by_s(int S, F f)
{
    switch (S) {
    case 1: return f(SConst<1>{});
    case 2: return f(SConst<2>{});
    case 3: return f(SConst<3>{});
    case 4: return f(SConst<4>{});
    default: return f(SConst<5>{});
    }
}

// k-blocks a wave of k_seq_gemm_p keeps in flight (K/V/R, ffn k/r at up to 4 KiB rows; a divisor of 8)
#ifndef RWKV_SEQ_DEPTH0
#define RWKV_SEQ_DEPTH0 2
#endif
#ifndef RWKV_SEQ_DEPTH2
#define RWKV_SEQ_DEPTH2 2
#endif
#ifndef RWKV_ATTOUT_R
#define RWKV_ATTOUT_R 2
#endif
constexpr int ATTOUT_R = RWKV_ATTOUT_R;
constexpr int SITE_NV[3] = {3, 2, 1};
constexpr int SQ_RING = 8;   // prompt chunks whose token ids may be in flight between host and device
constexpr int SITE_PW[3] = {site_pw<3>(), site_pw<2>(), site_pw<1>()};

template <typename K> int allow_smem(K kernel, size_t bytes)
{
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return 0;
}


// ---- argument blocks of the decode kernels ----
// (the stage's first ln1 site is opened by k_first's few workgroups, every other site by the full grid)
struct ArgMaker {
    rwkv_ctx *c;
    int D, grid, n_first;
    size_t LD;
    uint64_t wl(uint64_t l) const { return l - c->l0; }      // vectors are indexed by the model's layer, matrices by the stage's
    explicit ArgMaker(rwkv_ctx *c_) : c(c_), D((int)c_->D), grid(c_->grid), LD((size_t)c_->L * c_->D) { n_first = grid < 32 ? grid : 32; }
    unsigned long long *tl_of(int k, uint64_t l) const { return (c->tl_on && k == c->tl_cls && l == (c->l0 + c->l1) / 2) ? c->tl : nullptr; }
    SiteStatic site_static(int k, uint64_t ll) const
    {
        const int nv = SITE_NV[k], pw = SITE_PW[k];
        SiteStatic st;
        st.C = c->siteC[k] + (size_t)ll * nv * D; st.P = c->siteP[k] + (size_t)ll * D * pw;
        st.TC = c->siteTC[k] + (size_t)ll * nv; st.maxC = c->siteMC[k] + (size_t)ll * nv;
        st.invD = 1.0 / (double)D; st.invDm1 = 1.0 / (double)(D - 1);
        return st;
    }
    SiteDyn site_dyn(int k, int n_part) const
    {
        SiteDyn dy;
        dy.B = c->siteB[k]; dy.pd = c->sitePD[k]; dy.pf = c->sitePF[k]; dy.lnstat = c->lnstat + 2 * k; dy.n_part = n_part;
        return dy;
    }
    FirstArgs first() const
    {
        FirstArgs fa;
        fa.embed = c->embed; fa.ln = c->ln; fa.x = c->x; fa.x_in = c->x_in ? c->x_in : c->x; fa.st = site_static(0, c->l0); fa.dy = site_dyn(0, n_first);
        fa.sxy = c->state[0] + (size_t)c->l0 * D; fa.slot_stride = LD; fa.ctl = c->ctl; fa.D = D; fa.from_token = c->l0 == 0;
        return fa;
    }
    AttArgs att(uint64_t l) const
    {
        const size_t lo = (size_t)l * D;
        AttArgs aa;
        aa.x = c->x; aa.st = site_static(0, l); aa.dy = site_dyn(0, l == c->l0 ? n_first : grid);
        aa.w = c->wc[0].w_at(wl(l), D); aa.rs = c->wc[0].rs_at(wl(l), D);
        aa.uw = c->uw + lo; aa.ew = c->ew + lo;
        aa.r_att = c->attr + lo; aa.o_att = c->atto + lo;
        aa.saa = c->state[1] + lo; aa.sbb = c->state[2] + lo;
        aa.slot_stride = LD; aa.ybuf = c->ybuf; aa.partS = c->partA; aa.partM = c->partMA;
        aa.ctl = c->ctl; aa.D = D; aa.ns = 0; aa.tl = tl_of(1, l); aa.herr = c->d_herr;
        return aa;
    }
    AttOutArgs attout(uint64_t l) const
    {
        const size_t lo = (size_t)l * D;
        AttOutArgs ao;
        ao.w = c->wc[1].w_at(wl(l), D); ao.rs = c->wc[1].rs_at(wl(l), D); ao.ybuf = c->ybuf; ao.partS = c->partA; ao.partM = c->partMA; ao.n_part = grid;
        ao.x = c->x; ao.lnw = c->ln + (4 * l + 2) * D; ao.lnb = c->ln + (4 * l + 3) * D; ao.lnstat = c->lnstat + 0;
        ao.sxy = c->state[0] + lo; ao.st = site_static(1, l); ao.dy = site_dyn(1, grid); ao.sdd = c->state[4] + lo;
        ao.slot_stride = LD; ao.ctl = c->ctl; ao.D = D; ao.ns = 0; ao.tl = tl_of(2, l); ao.herr = c->d_herr;
        return ao;
    }
    FfnRKArgs frk(uint64_t l) const
    {
        const size_t lo = (size_t)l * D;
        FfnRKArgs fa;
        fa.x = c->x; fa.st = site_static(1, l); fa.dy = site_dyn(1, grid);
        fa.w = c->wc[2].w_at(wl(l), D); fa.rs = c->wc[2].rs_at(wl(l), D);
        fa.r_fv = c->fvr + 4 * lo; fa.o_fv = c->fvo + 4 * lo;
        fa.hbuf = c->hbuf; fa.rgate = c->rgate; fa.partS = c->partF; fa.partM = c->partMF; fa.ctl = c->ctl; fa.D = D;
        fa.ns = 0; fa.tl = tl_of(3, l); fa.herr = c->d_herr;
        return fa;
    }
    // the site ffn_v opens: ln1 of layer l + 1 (3 vectors), or ln_out -> head after the stage's last layer (on a non-final
    // pipeline stage nobody reads it: the next stage re-opens its own site from x)
    bool fv_next_att(uint64_t l) const { return l + 1 < c->l1; }
    FfnVArgs fv(uint64_t l) const
    {
        const size_t lo = (size_t)l * D;
        FfnVArgs fv;
        fv.w = c->wc[3].w_at(wl(l), D); fv.rs = c->wc[3].rs_at(wl(l), D); fv.hbuf = c->hbuf; fv.partS = c->partF; fv.partM = c->partMF; fv.n_part = grid;
        fv.rgate = c->rgate; fv.x = c->x; fv.lnw = c->ln + (4 * l + 4) * D; fv.lnb = c->ln + (4 * l + 5) * D; fv.lnstat = c->lnstat + 2;
        fv.sdd = c->state[4] + lo; fv.slot_stride = LD; fv.ctl = c->ctl; fv.D = D; fv.tl = tl_of(4, l);
        fv.ns = 0; fv.herr = c->d_herr;
        if (fv_next_att(l)) { fv.st = site_static(0, l + 1); fv.dy = site_dyn(0, grid); fv.sprev = c->state[0] + lo + D; }
        else { fv.st = site_static(2, 0); fv.dy = site_dyn(2, grid); fv.sprev = nullptr; }
        return fv;
    }
    HeadArgs head() const
    {
        HeadArgs ha;
        ha.x = c->x; ha.st = site_static(2, 0); ha.dy = site_dyn(2, grid); ha.w = c->wc[4].w; ha.rs = c->wc[4].rs; ha.logits = c->logits;
        ha.blk_val = c->blk_val; ha.blk_idx = c->blk_idx; ha.ctl = c->ctl; ha.D = D;
        return ha;
    }
};

// The decode kernels' instances, ONE table: which kernel runs a class for the context's configuration -- the tile form (tile_ok) at the context's
// tile instance, else the row form at S = ceil(D / 1024) -- with its dynamic LDS bytes (the kernels' own descriptions: tile.hip.h tile_lds_of,
// kernels.hip.h row_lds_of).  A = the row form's argument block, TA = the tile form's (A + the image); exactly one of row / tile is set.
// (The order of the functions and of the forms inside them is the order in which hipcc instantiates the kernels, and that is their order in the
// code object -- per class the tile instances, then the row instances, as it always was: profiles/decode_host/isa_compare.txt.)
template <class A, class TA = A> struct DecodeInst { void (*row)(A); void (*tile)(TA); size_t smem; };
DecodeInst<AttArgs, AttTArgs> att_inst(const rwkv_ctx *c)
{
    if (tile_ok(c, 1)) return {nullptr, by_tile(c, [](auto t) { using T = decltype(t); return &k_att_t<T::SD, T::S, T::KBT, T::TH, T::TPC>; }), tile_smem(c, 1)};
    return {by_s(c->S, [](auto s) { return &k_att<decltype(s)::value>; }), nullptr, row_lds_of(1, c->S).bytes};
}
DecodeInst<AttOutArgs, AttOutTArgs> attout_inst(const rwkv_ctx *c)
{
    if (tile_ok(c, 2)) return {nullptr, by_tile(c, [](auto t) { using T = decltype(t); return &k_attout_t<T::SD, T::S, T::KBT, T::TH, T::TPC>; }), tile_smem(c, 2)};
    return {by_s(c->S, [](auto s) { return &k_attout<decltype(s)::value, ATTOUT_R>; }), nullptr, row_lds_of(2, c->S).bytes};
}
DecodeInst<FfnRKArgs, FfnRKTArgs> frk_inst(const rwkv_ctx *c)
{
    if (tile_ok(c, 3)) return {nullptr, by_tile(c, [](auto t) { using T = decltype(t); return &k_ffn_rk_t<T::SD, T::S, T::KBT, T::TH, T::TPC>; }), tile_smem(c, 3)};
    return {by_s(c->S, [](auto s) { return &k_ffn_rk<decltype(s)::value>; }), nullptr, row_lds_of(3, c->S).bytes};
}
// ffn_v opens the next site: NVN = 3 vectors (ln1 of the next layer) or 1 (ln_out, ArgMaker::fv_next_att)
DecodeInst<FfnVArgs, FfnVTArgs> fv_inst(const rwkv_ctx *c, bool next_att)
{
    if (tile_ok(c, 4)) {
        const auto k3 = by_tile(c, [](auto t) { using T = decltype(t); return &k_ffnv_t<T::SD, T::S, T::KBT_FV, T::TH, T::TPC, 3>; });
        const auto k1 = by_tile(c, [](auto t) { using T = decltype(t); return &k_ffnv_t<T::SD, T::S, T::KBT_FV, T::TH, T::TPC, 1>; });
        return {nullptr, next_att ? k3 : k1, tile_smem(c, 4)};
    }
    const auto k3 = by_s(c->S, [](auto s) { return &k_ffnv<decltype(s)::value, 3>; });
    const auto k1 = by_s(c->S, [](auto s) { return &k_ffnv<decltype(s)::value, 1>; });
    return {next_att ? k3 : k1, nullptr, row_lds_of(4, c->S).bytes};
}
DecodeInst<HeadArgs> head_inst(const rwkv_ctx *c)      // (row form only)
{
    return {by_s(c->S, [](auto s) { return &k_head<decltype(s)::value>; }), nullptr, row_lds_of(5, c->S).bytes};
}
template <class A, class TA> int allow_smem(const DecodeInst<A, TA> &k) { return k.tile ? allow_smem(k.tile, k.smem) : allow_smem(k.row, k.smem); }

// ---- one launch helper per kernel class (0 embed, 1 att, 2 att_out, 3 ffn_rk, 4 ffn_v, 5 head, 6 argmax) ----
// a per-layer class: the instance's row form on the class's argument block, or its tile form on the block + the ring's length and the layer's image
template <class A, class TA> void launch_inst(rwkv_ctx *c, const DecodeInst<A, TA> &k, const A &a, int cls, uint64_t l)
{
    if (!k.tile) { k.row<<<dim3(c->grid), dim3(NT), k.smem, c->stream>>>(a); return; }
    TA ta;
    ta.a = a; ta.a.ns = tile_units(c, cls);
    ta.im.CB = (int)c->D / c->tile_th; ta.im.bimg = c->wc[cls - 1].t_at(l - c->l0, c->D);
    k.tile<<<dim3(c->grid), dim3(NT), k.smem, c->stream>>>(ta);
}
void launch_class(rwkv_ctx *c, int cls, uint64_t l)
{
    const ArgMaker mk(c);
    switch (cls) {
    case 0: {
        FirstArgs fa = mk.first();
        k_first<<<dim3(mk.n_first), dim3(NT), 0, c->stream>>>(fa);
    } break;
    case 1: launch_inst(c, att_inst(c), mk.att(l), 1, l); break;
    case 2: launch_inst(c, attout_inst(c), mk.attout(l), 2, l); break;
    case 3: launch_inst(c, frk_inst(c), mk.frk(l), 3, l); break;
    case 4: launch_inst(c, fv_inst(c, mk.fv_next_att(l)), mk.fv(l), 4, l); break;
    case 5: {
        const auto k = head_inst(c);
        k.row<<<dim3(c->grid), dim3(NT), k.smem, c->stream>>>(mk.head());
    } break;
    default:
        k_argmax_finish<<<dim3(1), dim3(64), 0, c->stream>>>(c->blk_val, c->blk_idx, c->grid, c->ctl, c->gen, c->gen_cap);
    }
}

// after a synchronisation: did a bounded wait inside a kernel give up?  (a tile-form LDS hand-off that never arrived: the GPU is
// shared or preempted, or a workgroup died.)  The token's results are not to be trusted: fail loudly instead of returning them.
// rc: the call has failed already -- the word is consumed all the same, the call's own status and message stay.
int device_check(rwkv_ctx *c, int rc = 0)
{
    if (!c->herr || *c->herr == 0u) return rc;
    const unsigned code = *c->herr;
    *c->herr = 0u;
    if (rc) return rc;
    return fail(RWKV_E_DEVICE, "a device-side wait gave up (code %u: an LDS hand-off timed out; is the GPU shared or preempted?) -- "
                               "the results of this call are invalid; RWKV_TILE=0 selects kernels without bounded waits", code);
}

// The exit of every synchronous entry point, with the status of what it enqueued (its downloads last): the context's stream is drained also
// when the call has failed -- what it did enqueue reads the pinned control blocks and the caller's arrays -- and the error word is consumed.
// The call's answer is the first failure: its own, the synchronisation's, the error word's.
int finish(rwkv_ctx *c, int rc)
{
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (!rc && e != hipSuccess) rc = fail(RWKV_E_DEVICE, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
    return device_check(c, rc);
}

// enqueue the kernels of one token on the context's stream.  ev: optional array of
// (4L + 4) events recorded before each launch and after the last (profiling).
int enqueue_token(rwkv_ctx *c, bool with_argmax, hipEvent_t *ev)
{
    const bool last = c->l1 == c->L;
    int evi = 0;
#define EV() do { if (ev) HIPCHK(hipEventRecord(ev[evi++], c->stream)); } while (0)
    EV();
    launch_class(c, 0, 0);   // first stage: embed + ln0; every stage: open the ln1 site of its first layer
    for (uint64_t l = c->l0; l < c->l1; l++)
        for (int cls = 1; cls <= 4; cls++) { EV(); launch_class(c, cls, l); }
    EV();
    if (last) launch_class(c, 5, 0);
    EV();
    if (last && with_argmax) launch_class(c, 6, 0);
    EV();
#undef EV
    HIPCHK(hipGetLastError());
    return 0;
}

int build_graph(rwkv_ctx *c, bool with_argmax, hipGraphExec_t *out)
{
    hipGraph_t g = nullptr;
    HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed));
    int rc = enqueue_token(c, with_argmax, nullptr);
    hipError_t e = hipStreamEndCapture(c->stream, &g);
    if (rc) return rc;
    HIPCHK(e);
    HIPCHK(hipGraphInstantiate(out, g, nullptr, nullptr, 0));
    HIPCHK(hipGraphDestroy(g));
    return 0;
}

// (re)capture the token graphs around the context's current argument blocks (x_in changes with rwkv_pipe_init / rwkv_pipe_free)
int rebuild_graphs(rwkv_ctx *c)
{
    int rc = 0;
    if (c->g_fwd) { (void)hipGraphExecDestroy(c->g_fwd); c->g_fwd = nullptr; rc = build_graph(c, false, &c->g_fwd); if (rc) { c->g_fwd = nullptr; return rc; } }
    if (c->g_greedy) { (void)hipGraphExecDestroy(c->g_greedy); c->g_greedy = nullptr; rc = build_graph(c, true, &c->g_greedy); if (rc) { c->g_greedy = nullptr; return rc; } }
    return 0;
}

int retile(rwkv_ctx *c, Source &src, int slot, uint64_t layer, uint64_t N, uint64_t M, uint8_t *dst,
           int G, int RS, int off, uint8_t *staging)
{
    const uint8_t *dsrc = static_cast<const uint8_t *>(src.device_ptr(slot, layer * N * M));
    if (!dsrc) {
        // `staging` is reused by the next matrix: stream order (this copy is enqueued behind the previous re-tile kernel) protects it
        int rc = src.to_device(slot, layer * N * M, N * M, staging, c->stream);
        if (rc) return rc;
        dsrc = staging;
    }
    dim3 grid((unsigned)((M + 63) / 64), (unsigned)((N + 63) / 64));
    hipLaunchKernelGGL(k_retile, grid, dim3(256), 0, c->stream, dsrc, dst, (int)N, (int)M, G, RS, off);
    HIPCHK(hipGetLastError());
    return 0;
}

template <typename T> int upload(rwkv_ctx *c, Source &src, int slot, T **dst)
{
    const uint64_t n = tensor_elems(slot, c->L, c->D);
    int rc = dalloc(c, dst, n);
    if (rc) return rc;
    // stream-ordered with the pack / re-tile kernels that read the copy (a default-stream D2D copy
    // would race with them: the engine stream is non-blocking)
    return src.to_device(slot, 0, n * sizeof(T), *dst, c->stream);
}

// The chunk path's GEMM instances, ONE table: which k_seq_gemm_p instance runs kind 0 K/V/R, 1 att_out, 2 ffn k/r, 3 ffn_v for a pass of one or
// two halves at octants of up to 8 k-blocks or more (`big`: D > 4096, the NKB = 10 instances), with its LDS bytes (the kernel's own description,
// seq.hip.h seq_lds_image) and the row tiles a wave has registers for.  Template arguments: TAG, NTW, NKB, NVS, DEPTH, MULTI, NH.
//  * two halves: both per weight fragment -- short k-block groups re-staged into the other LDS buffer (the image of two halves is twice as large;
//    twice the accumulators per weight tile);
//  * one half: the GEMM as a software pipeline over k-blocks, the slice's whole image resident (seq.hip.h k_seq_gemm_p) -- except ffn_v, whose
//    activation image (K = 4 D) is staged per 4 k-blocks into alternating LDS buffers instead of per slice, so that the first MFMA does not wait for
//    the whole slice's image (3.36 -> 3.30 ms per 7B chunk; for the other kinds it measured +-0 or a loss: profiles/r04/seq_small_ab.txt).
template <class A> struct SeqGemmInst { void (*fn)(A); size_t smem; int ntw; };
template <int TAG, int NTW, int NKB, int NVS, int DEPTH, bool MULTI, int NH> SeqGemmInst<SeqGemmArgs> seq_p_inst()
{
    return {k_seq_gemm_p<TAG, NTW, NKB, NVS, DEPTH, MULTI, NH>, seq_lds_image(MULTI ? 2 : 1, NH, NVS, NKB).bytes, NTW};
}
// (The order of the lines below is the order in which hipcc instantiates the kernels, and that is their order in the code object: one half before two,
// 8 k-blocks before 10, as it always was.  With the two-half instances first the SAME kernels ran a 32-token 7B chunk in 3.28 ms for 3.25,
// profiles/seq_gemm/ab.txt.)
SeqGemmInst<SeqGemmArgs> seq_gemm_p_for(int kind, bool two, bool big)
{
    if (!two) switch (kind) {
        case 0: return !big ? seq_p_inst<0, 3, 8, 3, RWKV_SEQ_DEPTH0, false, 1>() : seq_p_inst<0, 3, 10, 2, 2, false, 1>();
        case 1: return !big ? seq_p_inst<1, 1, 8, 1, 8, false, 1>() : seq_p_inst<1, 1, 10, 1, 10, false, 1>();
        case 2: return !big ? seq_p_inst<2, 5, 8, 2, RWKV_SEQ_DEPTH2, false, 1>() : seq_p_inst<2, 4, 10, 2, 2, false, 1>();
        default: return seq_p_inst<3, 1, 4, 1, 4, true, 1>();
    }
    switch (kind) {
        case 0: return seq_p_inst<0, 3, 2, 3, 2, true, 2>();
        case 1: return !big ? seq_p_inst<1, 1, 8, 1, 8, false, 2>() : seq_p_inst<1, 1, 10, 1, 10, false, 2>();
        case 2: return seq_p_inst<2, 3, 2, 2, 2, true, 2>();
        default: return seq_p_inst<3, 1, 4, 1, 4, true, 2>();
    }
}
// k_seq_gemm_b (two halves; kinds 0 and 2): `smem` is the largest launch, a slice of SEQ_B_NKB_MAX k-blocks; a launch asks for its own slice length
SeqGemmInst<SeqGemmBArgs> seq_gemm_b_for(int kind)
{
    const size_t smem = seq_lds_image(1, 2, 1, SEQ_B_NKB_MAX).bytes;
    if (kind == 0) return {k_seq_gemm_b<0, 3, RWKV_SEQ_BDEPTH, 2>, smem, 3};
    return {k_seq_gemm_b<2, 3, RWKV_SEQ_BDEPTH, 2>, smem, 3};
}
// How a context of width D with RWKV_SEQ_B = seq_b (-1: the default mask) launches GEMM `kind` in a pass of one or two halves: form, instance, grid
// and, for k_seq_gemm_b, the split of a slice's workgroups.  Plain host arithmetic over the two tables above: no context, no HIP call, no environment.
SeqGemmPlan seq_gemm_plan(int D, int seq_b, int kind, bool two)
{
    const SeqHalf h((size_t)D);
    const bool big = (D >> 6) > 8 * SEQ_O;       // octants of K = D longer than 8 k-blocks (D > 4096): the NKB = 10 instances
    // What follows from a GEMM's kind (0 K/V/R, 1 att_out, 2 ffn k/r, 3 ffn_v): row classes, K, the vector each class multiplies (padded with the
    // last), and where half 1 of the images and records it reads and of the partial values it writes lies
    struct GemmKind { int Q, K, voq[5]; size_t img_h, part_h, pk_h; };
    const GemmKind kinds[4] = {
        {3, D, {0, 1, 2, 2, 2}, h.img, h.part3, h.pk3},
        {1, D, {0, 0, 0, 0, 0}, h.img, h.part1, h.pk1},
        {5, D, {0, 0, 0, 0, 1}, h.img, h.part3, h.pk5},
        {1, 4 * D, {0, 0, 0, 0, 0}, h.imgh, h.part1, h.pk1},
    };
    const GemmKind &k = kinds[kind];
    const int Q = k.Q, N = Q * D, K = k.K;
    SeqGemmPlan p;
    SeqGemmArgs &g = p.args.g;
    g.N = N; g.K = K; g.Q = Q;
    for (int q = 0; q < 5; q++) g.vec_of_q[q] = k.voq[q];
    g.img_h = k.img_h / 4; g.part_h = k.part_h; g.pk_h = k.pk_h;      // (images: 16-byte units)
    const int nch = (N + Q - 1) / Q, ntiles = Q * ((nch + 15) / 16);
    if (two && (kind == 0 || kind == 2) && ((seq_b >= 0 ? seq_b : (4 | (D >= 4096 ? 1 : 0))) & (1 << kind))) {
        // k_seq_gemm_b: one vector's image of the slice resident, a wave's tiles in batches of <= 3.  The 32 workgroups of a slice are
        // shared out to the matrix's VECTOR GROUPS (runs of row classes on the same vector) so that no workgroup straddles one and the
        // largest tile count of a wave is as small as it gets.  Its conditions: slices of DEPTH .. SEQ_B_NKB_MAX k-blocks (the
        // resident image; row sums prefetched one batch ahead), at most three batches per wave, at most three groups
        const auto inst = seq_gemm_b_for(kind);
        const int KB = K >> 6, nkb_min = KB / SEQ_O, nkb_max = (KB + SEQ_O - 1) / SEQ_O, CBt = (nch + 15) / 16;
        SeqGemmBArgs b{};
        int ngrp = 0, gq[4] = {0, 0, 0, 0};
        for (int q = 0; q < Q && ngrp < 4; q++)
            if (q == 0 || k.voq[q] != k.voq[q - 1]) gq[ngrp++] = q;
        bool okb = ngrp <= 3 && nkb_min >= RWKV_SEQ_BDEPTH && nkb_max <= SEQ_B_NKB_MAX;
        if (okb) {
            int T[3] = {0, 0, 0}, best[3] = {0, 0, 0};
            for (int i = 0; i < ngrp; i++) { b.grp_tile[i] = gq[i] * CBt; T[i] = ((i + 1 < ngrp ? gq[i + 1] : Q) - gq[i]) * CBt; }
            b.grp_tile[ngrp] = ntiles;
            const int WG = 32;                 // workgroups per slice: 8 slices x 32 = one per CU
            double best_cost = 1e30;
            for (int w0 = 1; w0 <= WG; w0++)
                for (int w1 = (ngrp > 1 ? 1 : 0); w0 + w1 <= WG; w1 += 1) {
                    const int w2 = ngrp > 2 ? WG - w0 - w1 : 0;
                    if (ngrp == 1 && (w1 || w0 != WG)) continue;
                    if (ngrp == 2 && w0 + w1 != WG) continue;
                    if (ngrp == 3 && w2 < 1) continue;
                    const int w[3] = {w0, w1, w2};
                    double cost = 0;
                    for (int i = 0; i < ngrp; i++) {
                        const int per_wave = (T[i] + SEQ_NW * w[i] - 1) / (SEQ_NW * w[i]);
                        const double c2 = per_wave * 1000.0 + (double)T[i] / (SEQ_NW * w[i]);
                        if (c2 > cost) cost = c2;
                    }
                    if (cost < best_cost) { best_cost = cost; for (int i = 0; i < 3; i++) best[i] = w[i]; }
                    if (ngrp == 1) break;
                }
            int rb0 = 0, per_wave_max = 0;
            for (int i = 0; i < ngrp; i++) {
                b.grp_rb[i] = rb0; rb0 += best[i];
                const int pw = (T[i] + SEQ_NW * best[i] - 1) / (SEQ_NW * best[i]);
                if (pw > per_wave_max) per_wave_max = pw;
            }
            b.grp_rb[ngrp] = rb0; b.ngrp = ngrp;
            okb = per_wave_max <= 3 * inst.ntw && rb0 >= 1;
            if (okb) {
                b.g = g; b.g.ntw = per_wave_max;
                p.args = b; p.fn_b = inst.fn; p.smem = inst.smem; p.grid = SEQ_O * rb0; p.nkb_max = nkb_max;
                return p;
            }
        }
    }
    const auto inst = seq_gemm_p_for(kind, two, big);
    const int RB = (ntiles + SEQ_NW * inst.ntw - 1) / (SEQ_NW * inst.ntw);
    g.ntw = (ntiles + SEQ_NW * RB - 1) / (SEQ_NW * RB);
    p.fn_p = inst.fn; p.smem = inst.smem; p.grid = SEQ_O * RB;
    return p;
}
// the GEMM instances this context launches, and the head's, may ask for their dynamic LDS
int seq_smem_limits(const rwkv_ctx *c)
{
    int rc = allow_smem(k_seq_gemm_ks, seq_lds_ks().bytes);
    for (const SeqGemmPlan &p : c->seq_plan)
        if (!rc) rc = p.fn_b ? allow_smem(p.fn_b, p.smem) : allow_smem(p.fn_p, p.smem);
    return rc;
}
// one scratch set of the chunk path for the context's width: two halves of everything (SeqHalf), images and records zeroed
int alloc_scratch(rwkv_ctx *c, SeqScratch &S)
{
    const size_t D = c->D;
    const SeqHalf h(D);
    int rc = 0;
    auto zeroed = [&](auto **p, size_t count) -> int {
        if (const int e = dalloc(c, p, count)) return e;
        HIPCHK(hipMemsetAsync(*p, 0, count * sizeof(**p), c->stream));
        return 0;
    };
    if ((rc = dalloc(c, &S.state, D))) return rc;
    if ((rc = dalloc(c, &S.y, (size_t)SEQ_TM * D))) return rc;
    for (int k = 0; k < 3; k++)
        if ((rc = zeroed(&S.img[k], 2 * h.img))) return rc;
    if ((rc = zeroed(&S.imgh, 2 * h.imgh))) return rc;
    if ((rc = zeroed(&S.qpart, 2 * h.part3))) return rc;
    if ((rc = zeroed(&S.qparta, 2 * h.part1))) return rc;
    if ((rc = zeroed(&S.qparth, 2 * h.part1))) return rc;
    if ((rc = dalloc(c, &S.stat, (size_t)SEQ_TM * SEQ_O))) return rc;
    if ((rc = dalloc(c, &S.pk3, 2 * h.pk3))) return rc;
    if ((rc = dalloc(c, &S.pk5, 2 * h.pk5))) return rc;
    return dalloc(c, &S.pk1, 2 * h.pk1);
}

// the instances this context launches (its configuration is fixed by now) may ask for their dynamic LDS
int set_smem_limits(rwkv_ctx *c)
{
    int rc = allow_smem(att_inst(c));
    if (!rc) rc = allow_smem(attout_inst(c));
    if (!rc) rc = allow_smem(frk_inst(c));
    if (!rc) rc = allow_smem(fv_inst(c, true));
    if (!rc) rc = allow_smem(fv_inst(c, false));
    if (!rc) rc = allow_smem(head_inst(c));
    return rc;
}

int load_common(rwkv_ctx *c, Source &src, uint64_t L, uint64_t D, uint64_t max_ctx)
{
    if (c->loaded) return fail(RWKV_E_STATE, "RWKV already loaded");   // reference: rwkv.h:283-286
    if (L == 0 || D == 0 || D % 16 != 0 || D > 5120 || L > 4096)
        return fail(RWKV_E_ARG, "unsupported model shape n_layers=%llu n_embed=%llu (n_embed must be a multiple of 16, <= 5120)",
                    (unsigned long long)L, (unsigned long long)D);
    if (max_ctx == 0) max_ctx = 1;
    if ((uint64_t)c->grid * 512 < D)      // every decode kernel hands a workgroup its share of the D channels in groups of <= 512
        return fail(RWKV_E_ARG, "RWKV_GRID=%d is too small for n_embed=%llu (need >= %llu workgroups)", c->grid, (unsigned long long)D, (unsigned long long)((D + 511) / 512));
    HIPCHK(hipSetDevice(c->device));
    c->L = L; c->D = D; c->maxT = max_ctx; c->S = (int)((D + 1023) / 1024);
    if (c->l1 == UINT64_MAX) c->l1 = L;
    if (c->l0 >= c->l1 || c->l1 > L) return fail(RWKV_E_ARG, "layer range [%llu, %llu) does not fit a %llu-layer model", (unsigned long long)c->l0, (unsigned long long)c->l1, (unsigned long long)L);
    const uint64_t l0 = c->l0, l1 = c->l1, nl = l1 - l0;
    const bool first = l0 == 0, last = l1 == L;
    const uint64_t V = RWKV_VOCAB;
    int rc;

    // vectors: as-is
    if (first && (rc = upload(c, src, EMBED, &c->embed))) return rc;   // the table lives on the first stage only
    if ((rc = upload(c, src, LAYERNORMS, &c->ln))) return rc;
    if ((rc = upload(c, src, MIXK, &c->mixk))) return rc;
    if ((rc = upload(c, src, MIXV, &c->mixv))) return rc;
    if ((rc = upload(c, src, MIXR, &c->mixr))) return rc;
    if ((rc = upload(c, src, KR, &c->kr))) return rc;
    if ((rc = upload(c, src, VR, &c->vr))) return rc;
    if ((rc = upload(c, src, RR, &c->rr))) return rc;
    if ((rc = upload(c, src, O1, &c->o1))) return rc;
    if ((rc = upload(c, src, O2, &c->o2))) return rc;
    if ((rc = upload(c, src, O3, &c->o3))) return rc;
    if ((rc = upload(c, src, ATTOUTR, &c->attr))) return rc;
    if ((rc = upload(c, src, ATTOUTO, &c->atto))) return rc;
    if ((rc = upload(c, src, FFNMIXK, &c->fmixk))) return rc;
    if ((rc = upload(c, src, FFNMIXV, &c->fmixr))) return rc;   // slot named "v" holds time_mix_r
    if ((rc = upload(c, src, FFNKR, &c->fkr))) return rc;
    if ((rc = upload(c, src, FFNVR, &c->fvr))) return rc;
    if ((rc = upload(c, src, FFNRR, &c->frr))) return rc;
    if ((rc = upload(c, src, FFNKO, &c->fko))) return rc;
    if ((rc = upload(c, src, FFNVO, &c->fvo))) return rc;
    if ((rc = upload(c, src, FFNRO, &c->fro))) return rc;
    if ((rc = upload(c, src, HEADR, &c->headr))) return rc;
    if ((rc = upload(c, src, HEADO, &c->heado))) return rc;
    double *decay = nullptr, *bonus = nullptr;
    if ((rc = upload(c, src, DECAY, &decay))) return rc;
    if ((rc = upload(c, src, BONUS, &bonus))) return rc;
    if ((rc = dalloc(c, &c->uw, L * D))) return rc;
    if ((rc = dalloc(c, &c->ew, L * D))) return rc;
    hipLaunchKernelGGL(k_prep_wkv, dim3((unsigned)((L * D + 255) / 256)), dim3(256), 0, c->stream, decay, bonus, c->uw, c->ew, (size_t)(L * D));

    // LayerNorm-site tables for the layers of this stage (+ the head site)
    for (int k = 0; k < 3; k++) {
        const uint64_t n = k == 2 ? 1 : L;
        if ((rc = dalloc(c, &c->siteC[k], n * SITE_NV[k] * D))) return rc;
        if ((rc = dalloc(c, &c->siteP[k], n * D * SITE_PW[k]))) return rc;
        if ((rc = dalloc(c, &c->siteTC[k], n * SITE_NV[k]))) return rc;
        if ((rc = dalloc(c, &c->siteMC[k], n * SITE_NV[k]))) return rc;
        HIPCHK(hipMemsetAsync(c->siteP[k], 0, n * D * SITE_PW[k] * sizeof(float), c->stream));
    }
    {
        auto build = [&](int k, uint64_t ll, int m, const double *lnw, const double *lnb, const double *mix, const float *r, const float *o) {
            k_site_static<<<dim3(1), dim3(NT), 0, c->stream>>>(lnw, lnb, mix, r, o, c->siteC[k] + (size_t)ll * SITE_NV[k] * D,
                                                               c->siteP[k] + (size_t)ll * D * SITE_PW[k], c->siteTC[k] + (size_t)ll * SITE_NV[k],
                                                               c->siteMC[k] + (size_t)ll * SITE_NV[k], m, SITE_PW[k], (int)D);
        };
        for (uint64_t l = l0; l < l1; l++) {
            const size_t lo = (size_t)l * D;
            const double *w1 = c->ln + (4 * l + 2) * D, *b1 = c->ln + (4 * l + 3) * D, *w2 = c->ln + (4 * l + 4) * D, *b2 = c->ln + (4 * l + 5) * D;
            build(0, l, 0, w1, b1, c->mixk + lo, c->kr + lo, c->o1 + lo);
            build(0, l, 1, w1, b1, c->mixv + lo, c->vr + lo, c->o2 + lo);
            build(0, l, 2, w1, b1, c->mixr + lo, c->rr + lo, c->o3 + lo);
            build(1, l, 0, w2, b2, c->fmixk + lo, c->fkr + lo, c->fko + lo);
            build(1, l, 1, w2, b2, c->fmixr + lo, c->frr + lo, c->fro + lo);
        }
        build(2, 0, 0, c->ln + (4 * L + 2) * D, c->ln + (4 * L + 3) * D, nullptr, c->headr, c->heado);
        HIPCHK(hipGetLastError());
    }

    // uint8 matrices.  Two device layouts exist: ROW form -- re-tiled to row-per-output, what the row-form decode kernels
    // stream -- and the TILE image -- [16-row tile][k-block of 64][lane][16 B], signed: the MFMA B operand of the chunk path AND what the
    // tile-form decode kernels stream (tile.hip.h).  A decode class (K/V/R, att_out, ffn k/r, ffn_v: bits 0..3 of c->tile) is resident in
    // the ONE layout its decode kernel streams: the matrices of a class that runs in tile form go file layout -> row form in a scratch
    // buffer -> row sums, octant row sums, tile image, layer by layer, and their row form is never kept (7B-wide models on 256 CUs: all
    // four classes).  The 16-row tile image of every class is also what the chunk path (max_ctx > 1) multiplies with; at the widths whose
    // decode tiles are 4 rows high (tile.hip.h) a tile-form class has its own image.  The head stays in row form (k_head) either way
    // (+ its tile image for the chunk path).
    const bool want_seq = [&] { const char *e = getenv("RWKV_SEQ"); return max_ctx > 1 && D % 64 == 0 && !(e && e[0] == '0'); }();
    const TileCfg tcfg = tile_cfg_for(D, c->grid);
    // auto: every class where a workgroup owns exactly one 16-channel block (D = 4096) and, on 4-row tiles, at D = 5120; K/V/R, ffn k/r and ffn_v at
    // D = 2048 (att_out: 4.8 us in row form, 5.2 in tile form).  Measured per mask with round 6's per-class heads and matrix-core consumers
    // (profiles/r06/tile_masks_ab.txt: 14B 345.7 -> 365 tokens/s, 1B5 1345 -> 1417); round 5's kernels had every class but 14B's ffn k/r faster in row form.
    if (c->tile < 0) c->tile = tcfg.th == 16 || tcfg.tpc == 5 ? 15 : tcfg.tpc == 2 ? 13 : 0;
    if (tcfg.th == 0) c->tile = 0;
    c->tile &= 15;
    if (c->tile) { c->tile_th = tcfg.th; c->tile_s = tcfg.s; c->tile_tpc = tcfg.tpc; }
    auto in_tile = [&](int cls) { return ((c->tile >> (cls - 1)) & 1) != 0; };
    const bool own_t = tcfg.th != 16;                         // the decode kernels' tile image is not the chunk path's
    auto need_b = [&](int cls) { return want_seq || (in_tile(cls) && !own_t); };
    WClass *const wc = c->wc, &head = c->wc[4];
    // (all row forms, then all row sums, images, octant row sums, decode-only images: the order of the allocations is the order of the addresses)
    for (int k = 0; k < 4; k++)
        if (!in_tile(k + 1) && (rc = dalloc(c, &wc[k].w, nl * wc[k].row_bytes(D)))) return rc;
    if (last && (rc = dalloc(c, &head.w, head.row_bytes(D)))) return rc;
    for (int k = 0; k < 5; k++)
        if ((rc = dalloc(c, &wc[k].rs, (k < 4 ? nl : 1) * wc[k].sums(D)))) return rc;
    for (int k = 0; k < 4; k++)
        if (need_b(k + 1) && (rc = dalloc(c, &wc[k].b, nl * wc[k].img_bytes(D)))) return rc;
    for (int k = 0; k < 4 && want_seq; k++)
        if ((rc = dalloc(c, &wc[k].r8, nl * wc[k].sums8(D)))) return rc;
    for (int k = 0; k < 4; k++) {
        if (!in_tile(k + 1)) continue;
        if (!own_t) wc[k].t = wc[k].b;
        else if ((rc = dalloc(c, &wc[k].t, nl * wc[k].row_bytes(D)))) return rc;
    }
    // load-time scratch (not part of the context): freed on every way out of this function, behind the stream's work
    struct Scratch {
        hipStream_t st; uint8_t *p = nullptr;
        ~Scratch() { if (p) { (void)hipStreamSynchronize(st); (void)hipFree(p); } }
    } staging_s{c->stream}, rowtmp_s{c->stream};
    if (!src.on_device) HIPCHK(hipMalloc(reinterpret_cast<void **>(&staging_s.p), std::max<uint64_t>(4 * D * D, V * D)));
    if (c->tile) HIPCHK(hipMalloc(reinterpret_cast<void **>(&rowtmp_s.p), wc[2].row_bytes(D)));      // one layer of the largest class
    uint8_t *const staging = staging_s.p, *const rowtmp = rowtmp_s.p;
    // One layer (wl of the stage, l of the model) of one class: its file tensors -> row form at `row` -> row sums, and from the row form
    // (w_t[N][K]) the image of 16-row tiles with its octant row sums, and the decode-only image of TH-row tiles
    auto image = [&](const uint8_t *w_t, uint8_t *dst, const WClass &k, int TH) {
        const uint64_t tiles = k.Q * ((k.rows(D) + TH - 1) / TH);
        k_bimage<<<dim3((unsigned)((tiles * TH * k.K(D) / 16 + 255) / 256)), dim3(256), 0, c->stream>>>(w_t, dst, (int)k.N(D), (int)k.K(D), k.Q, (int)(tiles / k.Q), TH);
    };
    auto build = [&](WClass &k, uint64_t l, uint64_t wl, uint8_t *row, bool with_b, bool with_t) -> int {
        for (int i = 0; i < k.nsrc; i++) {
            const WSrc &f = k.src[i];
            if (const int e = retile(c, src, f.slot, l, f.n * D, f.m ? f.m * D : V, row, f.G, f.RS, f.off, staging)) return e;
        }
        k_rowsum<<<dim3((unsigned)((k.N(D) + 3) / 4)), dim3(256), 0, c->stream>>>(row, k.rs + wl * k.sums(D), (size_t)k.N(D), (int)k.K(D));
        if (with_b) image(row, k.b + wl * k.img_bytes(D), k, 16);
        if (with_b && k.r8) k_rowsum8<<<dim3((unsigned)((k.N(D) + 3) / 4)), dim3(256), 0, c->stream>>>(row, k.r8 + wl * k.sums8(D), (int)k.N(D), (int)k.K(D));
        if (with_t) image(row, k.t + wl * k.row_bytes(D), k, tcfg.th);
        return 0;
    };
    for (uint64_t l = l0; l < l1 && !rc; l++)
        for (int k = 0; k < 4 && !rc; k++)
            rc = build(wc[k], l, l - l0, in_tile(k + 1) ? rowtmp : wc[k].w + (l - l0) * wc[k].row_bytes(D), need_b(k + 1), own_t && in_tile(k + 1));
    if (!rc && last) {      // the head stays in row form (k_head); its image is the chunk path's alone
        if (want_seq && !(rc = dalloc(c, &head.b, head.img_bytes(D)))) rc = dalloc(c, &head.r8, head.sums8(D));
        if (!rc) rc = build(head, 0, 0, head.w, want_seq, false);
    }
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipGetLastError());

    // state (zero, as `new RWKVState` does: rwkv.h:163-170) and scratch
    for (int s = 0; s < 5; s++) {
        if ((rc = dalloc(c, &c->state[s], max_ctx * L * D))) return rc;
        HIPCHK(hipMemsetAsync(c->state[s], 0, max_ctx * L * D * sizeof(double), c->stream));
    }
    if ((rc = dalloc(c, &c->x, D))) return rc;
    for (int k = 0; k < 3; k++) {
        if ((rc = dalloc(c, &c->siteB[k], (size_t)SITE_NV[k] * D))) return rc;
        if ((rc = dalloc(c, &c->sitePD[k], (size_t)c->grid * 8))) return rc;
        if ((rc = dalloc(c, &c->sitePF[k], (size_t)c->grid * 4))) return rc;
        HIPCHK(hipMemsetAsync(c->sitePD[k], 0, (size_t)c->grid * 8 * sizeof(double), c->stream));
        HIPCHK(hipMemsetAsync(c->sitePF[k], 0, (size_t)c->grid * 4 * sizeof(float), c->stream));
    }
    if ((rc = dalloc(c, &c->lnstat, 6))) return rc;
    if ((rc = dalloc(c, &c->ybuf, D))) return rc;
    if ((rc = dalloc(c, &c->hbuf, 4 * D))) return rc;
    if ((rc = dalloc(c, &c->rgate, D))) return rc;
    if ((rc = dalloc(c, &c->partA, (size_t)c->grid))) return rc;
    if ((rc = dalloc(c, &c->partF, (size_t)c->grid))) return rc;
    if ((rc = dalloc(c, &c->partMA, (size_t)c->grid))) return rc;
    if ((rc = dalloc(c, &c->partMF, (size_t)c->grid))) return rc;
    if ((rc = dalloc(c, &c->blk_val, (size_t)c->grid))) return rc;
    if ((rc = dalloc(c, &c->blk_idx, (size_t)c->grid))) return rc;
    if ((rc = dalloc(c, &c->logits, max_ctx * V))) return rc;
    HIPCHK(hipMemsetAsync(c->logits, 0, max_ctx * V * sizeof(float), c->stream));
    if ((rc = dalloc(c, &c->ctl, 1))) return rc;
    HIPCHK(hipMemsetAsync(c->ctl, 0, sizeof(Ctl), c->stream));
    HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&c->h_ctl), sizeof(Ctl) * max_ctx, hipHostMallocDefault));
    constexpr unsigned GEN_CAP = 1u << 16;
    static_assert(GEN_CAP == RWKV_MAX_DECODE_STEPS, "the one-stream form of a generation call writes gen[k] for every k < n_steps");
    c->gen_cap = GEN_CAP;
    if ((rc = dalloc(c, &c->gen, (size_t)c->gen_cap))) return rc;
    HIPCHK(hipMemsetAsync(c->gen, 0, (size_t)c->gen_cap * sizeof(unsigned long long), c->stream));
    if ((rc = dalloc(c, &c->pick, 1))) return rc;
    if ((rc = dalloc(c, &c->ts_part, (size_t)TS_G * 3))) return rc;
    if ((rc = dalloc(c, &c->ts_p, (size_t)TS_NT * TS_PER))) return rc;
    if ((rc = dalloc(c, &c->ts_pw, (size_t)TS_NT * TS_PER))) return rc;
    if ((rc = dalloc(c, &c->ts_key, (size_t)TS_NT * TS_PER))) return rc;

    // chunked path scratch
    {
        if (want_seq) {
            // k_seq_resid covers its octant with three channels per thread (seq.hip.h SEQ_RJ): the longest octant has to fit
            if ((D / 64 + 7) / 8 * 64 > 3 * (uint64_t)SEQ_ENT)
                return fail(RWKV_E_ARG, "n_embed=%llu: an octant of the chunk path is longer than %d channels", (unsigned long long)D, 3 * SEQ_ENT);
            if ((rc = dalloc(c, &c->sq_tokens, (size_t)SQ_RING * SEQ_TM))) return rc;
            HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&c->h_sq_tokens), sizeof(unsigned long long) * SQ_RING * SEQ_TM, hipHostMallocDefault));
            for (int r = 0; r < SQ_RING; r++) HIPCHK(hipEventCreateWithFlags(&c->sq_ev[r], hipEventDisableTiming));
            if ((rc = dalloc(c, &c->sq_x[0], (size_t)SEQ_TM * D))) return rc;
            if ((rc = dalloc(c, &c->sq_x[1], (size_t)SEQ_TM * D))) return rc;
            if ((rc = alloc_scratch(c, c->sp_scratch[0]))) return rc;
            for (int i = 0; i < 8; i++) c->seq_plan[i] = seq_gemm_plan((int)D, c->seq_b, i & 3, i >> 2);
            c->sp_stream[0] = c->stream;
            c->seq_ok = true;
        }
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    if ((rc = set_smem_limits(c))) return rc;
    if (c->seq_ok && (rc = seq_smem_limits(c))) return rc;
    if (c->graphs & 1) {
        if ((rc = build_graph(c, false, &c->g_fwd))) return rc;
        if ((rc = build_graph(c, true, &c->g_greedy))) return rc;
    }
    c->loaded = true;
    return 0;
}

// The ROW LAYOUT of a pass: what its rows are to each other -- one of four, with the one thing that layout needs besides the pass's rows.
//   GPT        rwkv.cu:493-593: n tokens of one sequence on state slot 0, the token shift runs along the rows
//   PARRALEL   rwkv.cu:236-240: n independent sequences, one token each, row t on state slot row0 + t -- the batched decode step
//   CKPT       the verify pass of rwkv_spec_verify (spec.hip.h): GPT rows, one half, whole model, that commit NOTHING to slot 0 -- every row's state
//              is left in `ckpt`, [4][L][n][D]
//   SEGMENTED  segments.hip.h: the rows are pieces of sequences on slots of their own, as `plan` says ([rows]{slot, flags} on the device)
// Only GPT passes are replayed as captured graphs (enqueue_pass: its key holds a shape, no layout); the rest change from call to call and are
// launched directly.
struct RowLayout {
    enum Kind { GPT, PARRALEL, CKPT, SEGMENTED } kind = GPT;
    union { double *ckpt = nullptr; const SegRow *plan; };
    static RowLayout of_mode(int mode) { RowLayout r; r.kind = mode == RWKV_MODE_PARRALEL ? PARRALEL : GPT; return r; }
    static RowLayout checkpoints(double *ck) { RowLayout r; r.kind = CKPT; r.ckpt = ck; return r; }
    static RowLayout segments(const SegRow *plan) { RowLayout r; r.kind = SEGMENTED; r.plan = plan; return r; }
    bool replayed() const { return kind == GPT; }
    RowLayout from_row(uint64_t t0) const { RowLayout r = *this; if (kind == SEGMENTED) r.plan += t0; return r; }      // the layout of the pass that starts at row t0 of a call
};
// One pass (n <= SEQ_TM = 64 rows: one or two halves of <= 32) through the MFMA path (seq.hip.h) for layers [la, lb) of THIS context's [l0, l1);
// logits rows [row0, row0 + n) where the pass holds the head.
// The residual stream of the chunk lives in sq_x[buf]: the pass that holds the embedding fills it from the table, a later
// pipeline stage finds the previous stage's output there (placed by an RCCL recv or a copy) and every stage leaves its
// own output in it.  The layers run on `st` with scratch set `S` (the software pipeline of rwkv_forward: a stream and a set per stage).
// dtok: the pass's n token ids on the device, read where the pass holds the embedding -- token_slot(c, buf) behind upload_chunk_tokens, or wherever
// they already are (the batched decode's picks of the previous step)
struct SeqPass {
    uint64_t la, lb; hipStream_t st; const SeqScratch *S; int buf, n; uint64_t row0; const unsigned long long *dtok; RowLayout rows;
    bool embeds(const rwkv_ctx *c) const { return c->l0 == 0 && la == c->l0; }
    bool heads(const rwkv_ctx *c) const { return c->l1 == c->L && lb == c->l1; }
};
unsigned long long *token_slot(const rwkv_ctx *c, int buf) { return c->sq_tokens + (size_t)buf * SEQ_TM; }
// a pass's token ids: host -> pinned ring slot -> the device slot of the pass's residual buffer (the copy is stream-ordered behind the
// embedding kernel of the pass that used the buffer before).  Nothing here waits for the device: the ids go through a ring of pinned slots.
int upload_chunk_tokens(rwkv_ctx *c, const uint64_t *tokens, int n, int buf, hipStream_t st)
{
    const int slot = (int)(c->sq_n % SQ_RING);
    if (c->sq_n >= SQ_RING) HIPCHK(hipEventSynchronize(c->sq_ev[slot]));   // the copy that last used this pinned slot is done
    unsigned long long *h = c->h_sq_tokens + (size_t)slot * SEQ_TM;
    for (int t = 0; t < n; t++) h[t] = tokens[t];
    HIPCHK(hipMemcpyAsync(token_slot(c, buf), h, sizeof(unsigned long long) * n, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(c->sq_ev[slot], st));
    c->sq_n++;
    return 0;
}
// The instances of the CKPT and SEGMENTED layouts are declared here and NAMED beside their features, behind every other kernel: hipcc emits a template
// instance where host code first names it, and a kernel that moves in the code object costs time elsewhere (beam.hip.h k_beam_select).
struct SeqCkptFns { void (*site3)(SeqSiteArgs) = nullptr; void (*site2)(SeqSiteArgs) = nullptr; void (*wkv)(SeqWkvArgs) = nullptr; };
SeqCkptFns seq_ckpt_fns();
struct SegFns {
    void (*site3)(SegSiteArgs) = nullptr; void (*site2)(SegSiteArgs) = nullptr; void (*wkv32)(SegWkvArgs) = nullptr; void (*wkv64)(SegWkvArgs) = nullptr;
    void (*stage)(SegStageArgs) = nullptr;
};
SegFns seg_fns();
int enqueue_chunk(rwkv_ctx *c, const SeqPass &pass)
{
    if (pass.buf < 0 || pass.buf >= rwkv_ctx::SPLIT_MAX) return fail(RWKV_E_ARG, "residual buffer %d out of range", pass.buf);
    const int D = (int)c->D, n = pass.n;
    const uint64_t L = c->L, V = RWKV_VOCAB, row0 = pass.row0;
    hipStream_t st = pass.st;
    const SeqScratch &S = *pass.S;
    double *x = c->sq_x[pass.buf];
    if (pass.embeds(c)) {
        SeqEmbedArgs ea{c->embed, c->ln, pass.dtok, x, D};
        k_seq_embed<<<dim3(n), dim3(NT), 0, st>>>(ea);
    }
    const size_t LD = (size_t)L * D;
    const int egrid = n * SEQ_O;
    // a pass of 33 .. 64 rows has two halves (seq.hip.h SEQ_TM): the GEMMs read the weights ONCE for both, everything per half sits
    // at these element offsets behind half 0's
    const bool two = n > SEQ_T;
    const SeqHalf h((size_t)D);
    // What the layout means, said once.  A site with a token shift keeps its LayerNorm output for the sequence's next row: GPT in S.state (the last
    // row's), which the GEMM behind the site copies to slot 0 (`commits`); PARRALEL in the row's own slot; CKPT in the checkpoint rows; SEGMENTED in
    // the staging rows, which the WKV and stage-1 kernels behind the GEMMs commit.  The three launch helpers below (site, wkv, stage) pick their instance.
    const RowLayout &rows = pass.rows;
    const bool commits = rows.kind == RowLayout::GPT;
    if (rows.kind == RowLayout::CKPT && two) return fail(RWKV_E_ARG, "a checkpointing pass is one half");
    if (rows.kind == RowLayout::SEGMENTED && !S.seg) return fail(RWKV_E_ARG, "the scratch set of a segmented pass holds the staging rows");
    const SeqCkptFns ckf = rows.kind == RowLayout::CKPT ? seq_ckpt_fns() : SeqCkptFns{};
    const SegFns sgf = rows.kind == RowLayout::SEGMENTED ? seg_fns() : SegFns{};
    const size_t ck_arr = (size_t)L * n * D;      // one of the four checkpoint arrays; layer l's rows start l * n * D into it
    bool tl_layer = false;     // debug timeline (rwkv_debug_timeline with RWKV_TL_CLASS = 10 + GEMM kind): the middle layer's GEMM stamps its phases
    // the records a GEMM of each kind (0 K/V/R, 1 att_out, 2 ffn k/r, 3 ffn_v) reads and the partial values it writes, in the pass's scratch set
    const SeqPart *const parts[4] = {S.qpart, S.qparta, S.qpart, S.qparth};
    float *const pks[4] = {S.pk3, S.pk1, S.pk5, S.pk1};
    // tile-per-wave GEMM of layer matrix `bimg` (row sums `rs8`) over the 8 K-slices, partial values into the kind's pk, launched as the context's
    // plan says (seq_gemm_plan); state_dst: where a layout that `commits` has it copy the state of the site in front of it
    auto gemm = [&](int kind, const uint8_t *bimg, const unsigned *rs8, double *state_dst) {
        const SeqGemmPlan &p = c->seq_plan[4 * two + kind];
        SeqGemmBArgs b = p.args;
        SeqGemmArgs &g = b.g;
        g.bimg = reinterpret_cast<const u32x4 *>(bimg); g.rs8 = rs8;
        for (int v = 0; v < 3; v++) g.img[v] = reinterpret_cast<const u32x4 *>(kind == 3 ? S.imgh : S.img[v]);
        g.part = parts[kind]; g.pk = pks[kind]; g.out = nullptr; g.T = n;
        g.tl = (c->tl_on && c->tl_cls == 10 + kind && tl_layer) ? c->tl : nullptr;
        g.cp_src = S.state; g.cp_dst = state_dst; g.cp_n = (state_dst && commits) ? D : 0;
        if (p.fn_b) p.fn_b<<<dim3(p.grid), dim3(SEQ_NT), seq_lds_image(1, 2, 1, p.nkb_max).bytes, st>>>(b);
        else p.fn_p<<<dim3(p.grid), dim3(SEQ_NT), p.smem, st>>>(g);
    };
    auto resid = [&](int mode, const SeqPart *qpart) {
        SeqResidArgs r{};
        r.x = x; r.pk = S.pk1; r.qpart = qpart; r.pk_gate = S.pk5; r.qpart_gate = S.qpart + (size_t)1 * SEQ_T * SEQ_O;   // ffn r = vector 1 of the ln2 site
        r.stat = S.stat; r.D = D; r.T = n;
        r.pk_h = h.pk1; r.pkg_h = h.pk5; r.part_h = h.part1; r.partg_h = h.part3;
        if (mode == 0) k_seq_resid<0><<<dim3(egrid), dim3(SEQ_ENT), 0, st>>>(r);
        else if (mode == 1) k_seq_resid<1><<<dim3(egrid), dim3(SEQ_ENT), 0, st>>>(r);
        else k_seq_resid<2><<<dim3(egrid), dim3(SEQ_ENT), 0, st>>>(r);
    };
    // state: this layer's xy / dd of slot 0 for a site with a token shift, null for ln_out, which shifts and keeps nothing and so is the plain instance
    // in every layout; ck_at: where this site's rows start in the checkpoint arrays
    auto site = [&](int nv, const double *lnw, const double *lnb, const double *const *mix, const float *const *r, const float *const *o, double *state, size_t ck_at) {
        SeqSiteArgs s{};
        s.x = x; s.stat = S.stat; s.lnw = lnw; s.lnb = lnb;
        for (int q = 0; q < nv; q++) { s.mix[q] = mix ? mix[q] : nullptr; s.r[q] = r[q]; s.o[q] = o[q]; }
        s.state = s.state_par = state; s.slot_stride = LD; s.slot0 = (int)row0;
        for (int q = 0; q < 3; q++) s.img[q] = S.img[q];
        s.part = S.qpart; s.D = D; s.T = n;
        s.img_h = h.img; s.part_h = h.part3;
        const dim3 grid(egrid), block(SEQ_ENT);
        switch (state ? rows.kind : RowLayout::GPT) {
        case RowLayout::SEGMENTED: (nv == 3 ? sgf.site3 : sgf.site2)<<<grid, block, 0, st>>>(SegSiteArgs{s, rows.plan, S.seg}); return;
        case RowLayout::CKPT: s.ckpt = rows.ckpt + ck_at; (nv == 3 ? ckf.site3 : ckf.site2)<<<grid, block, 0, st>>>(s); return;
        case RowLayout::PARRALEL: s.par = 1; break;
        case RowLayout::GPT: s.state_new = state ? S.state : nullptr; break;      // (and ln_out of every layout: nothing to keep)
        }
        if (nv == 3) k_seq_site<3><<<grid, block, 0, st>>>(s);
        else if (nv == 2) k_seq_site<2><<<grid, block, 0, st>>>(s);
        else k_seq_site<1><<<grid, block, 0, st>>>(s);
    };
    auto wkv = [&](size_t lo) {
        SeqWkvArgs wa{S.pk3, S.qpart, c->uw + lo, c->ew + lo, c->state[1] + lo, c->state[2] + lo, S.y, D, n, rows.kind == RowLayout::PARRALEL, LD, (int)row0, h.pk3, h.part3};
        const dim3 grid((D + WKV_CH - 1) / WKV_CH), block((two ? SEQ_TM : SEQ_T) * WKV_CH);
        switch (rows.kind) {
        case RowLayout::SEGMENTED: (two ? sgf.wkv64 : sgf.wkv32)<<<grid, block, 0, st>>>(SegWkvArgs{wa, rows.plan, S.seg, c->state[0] + lo}); return;
        case RowLayout::CKPT:      // (one half: refused above otherwise)
            wa.ckpt_aa = rows.ckpt + ck_arr + lo * n; wa.ckpt_bb = rows.ckpt + 2 * ck_arr + lo * n;
            ckf.wkv<<<grid, block, 0, st>>>(wa);
            return;
        default: break;
        }
        if (two) k_seq_wkv<SEQ_TM><<<grid, block, 0, st>>>(wa);
        else k_seq_wkv<SEQ_T><<<grid, block, 0, st>>>(wa);
    };
    // kind 0: the att_out input, the same in every layout; kind 1: the ffn_v input -- in a segmented pass with the commit of the ln2 site's rows
    auto stage = [&](int kind, const SeqStageArgs &sa, size_t lo) {
        const dim3 grid(egrid), block(SEQ_ENT);
        if (kind == 0) k_seq_stage<0><<<grid, block, 0, st>>>(sa);
        else if (rows.kind == RowLayout::SEGMENTED) sgf.stage<<<grid, block, 0, st>>>(SegStageArgs{sa, rows.plan, S.seg, c->state[4] + lo, LD, D});
        else k_seq_stage<1><<<grid, block, 0, st>>>(sa);
    };
    resid(0, nullptr);     // LayerNorm statistics of the incoming residual stream (embedding rows, or the previous stage's output)
    for (uint64_t l = pass.la; l < pass.lb; l++) {
        tl_layer = l == (c->l0 + c->l1) / 2;
        const size_t lo = (size_t)l * D;
        const uint64_t wl = l - c->l0;   // vectors are indexed by the model's layer, matrices by the stage's
        {   // time mix
            const double *mix[3] = {c->mixk + lo, c->mixv + lo, c->mixr + lo};
            const float *r[3] = {c->kr + lo, c->vr + lo, c->rr + lo}, *o[3] = {c->o1 + lo, c->o2 + lo, c->o3 + lo};
            site(3, c->ln + (4 * l + 2) * D, c->ln + (4 * l + 3) * D, mix, r, o, c->state[0] + lo, lo * n);
            gemm(0, c->wc[0].b_at(wl, D), c->wc[0].r8_at(wl, D), c->state[0] + lo);
            wkv(lo);
            SeqStageArgs sa{S.y, nullptr, nullptr, c->attr + lo, c->atto + lo, S.img[0], S.qparta, D, n, 0, 0, h.img, h.part1};
            stage(0, sa, lo);
            gemm(1, c->wc[1].b_at(wl, D), c->wc[1].r8_at(wl, D), nullptr);
            // x = f32(x) + att_out; statistics for ln2.  (Round 3 tried this launch and the site behind it as ONE launch whose (row, octant)
            // workgroups meet on a per-row arrival counter: +3.6 us per fused launch, profiles/r03/prefill_fuse.txt -- the in-launch
            // all-to-all costs more than the kernel boundary it replaces.)
            resid(1, S.qparta);
        }
        {   // channel mix
            const double *mix[3] = {c->fmixk + lo, c->fmixr + lo, nullptr};
            const float *r[3] = {c->fkr + lo, c->frr + lo, nullptr}, *o[3] = {c->fko + lo, c->fro + lo, nullptr};
            site(2, c->ln + (4 * l + 4) * D, c->ln + (4 * l + 5) * D, mix, r, o, c->state[4] + lo, 3 * ck_arr + lo * n);
            gemm(2, c->wc[2].b_at(wl, D), c->wc[2].r8_at(wl, D), c->state[4] + lo);
            SeqStageArgs sh{nullptr, S.pk5, S.qpart, c->fvr + 4 * lo, c->fvo + 4 * lo, S.imgh, S.qparth, 4 * D, n, h.pk5, h.part3, h.imgh, h.part1};
            stage(1, sh, lo);
            gemm(3, c->wc[3].b_at(wl, D), c->wc[3].r8_at(wl, D), nullptr);
            resid(2, S.qparth);     // x += ffn_v * sigmoid(r); statistics for the next site
        }
    }
    if (pass.heads(c)) {   // ln_out and the head
        const float *r[3] = {c->headr, nullptr, nullptr}, *o[3] = {c->heado, nullptr, nullptr};
        site(1, c->ln + (4 * L + 2) * D, c->ln + (4 * L + 3) * D, nullptr, r, o, nullptr, 0);
        SeqGemmArgs g{};
        g.bimg = reinterpret_cast<const u32x4 *>(c->wc[4].b); g.rs8 = c->wc[4].r8; g.N = (int)V; g.K = D; g.Q = 1;
        for (int hf = 0; hf < (two ? 2 : 1); hf++) {      // the head once per half (its weights are 3 % of a pass's bytes; 240 accumulator registers would not fit one wave)
            for (int k = 0; k < 3; k++) g.img[k] = reinterpret_cast<const u32x4 *>(S.img[k] + hf * h.img);
            g.part = S.qpart + hf * h.part3; g.out = c->logits + (row0 + hf * SEQ_T) * V; g.T = hf ? n - SEQ_T : (two ? SEQ_T : n);
            k_seq_gemm_ks<<<dim3(c->grid), dim3(SEQ_NT), seq_lds_ks().bytes, st>>>(g);
        }
    }
    HIPCHK(hipGetLastError());
    return 0;
}
// a GPT-mode pass over the context's whole layer range on its own stream with its own scratch, the ids (where it holds the embedding) from the host
int enqueue_whole(rwkv_ctx *c, const uint64_t *tokens, int n, uint64_t row0, int buf)
{
    const SeqPass pass{c->l0, c->l1, c->stream, &c->sp_scratch[0], buf, n, row0, token_slot(c, buf)};
    if (pass.embeds(c)) { const int rcu = upload_chunk_tokens(c, tokens, n, buf, c->stream); if (rcu) return rcu; }
    return enqueue_chunk(c, pass);
}

// the chunk path's software pipeline on one GPU: streams, events, one more scratch set and residual-stream buffer per extra
// stage (allocated at first use: 40 MB per stage at 7B).  RWKV_SEQ_STAGES = 1 .. 4 (default 3; 1 = the one-stream schedule)
int split_setup(rwkv_ctx *c)
{
    if (c->n_split) return 0;
    int want = 3;
    if (const char *e = getenv("RWKV_SEQ_STAGES")) want = atoi(e);
    if (want > rwkv_ctx::SPLIT_MAX) want = rwkv_ctx::SPLIT_MAX;
    if ((uint64_t)want > c->L) want = (int)c->L;
    if (want < 2 || !c->seq_ok || c->l0 != 0 || c->l1 != c->L) { c->n_split = 1; return 0; }
    HIPCHK(hipEventCreateWithFlags(&c->sp_end, hipEventDisableTiming));
    for (int k = 0; k < want; k++) {
        if (k > 0) HIPCHK(hipStreamCreateWithFlags(&c->sp_stream[k], hipStreamNonBlocking));
        for (int b = 0; b < want; b++) HIPCHK(hipEventCreateWithFlags(&c->sp_done[k][b], hipEventDisableTiming));
    }
    int rc = 0;
    for (int k = 2; k < want && !rc; k++) rc = dalloc(c, &c->sq_x[k], (size_t)SEQ_TM * c->D);
    for (int k = 1; k < want && !rc; k++) rc = alloc_scratch(c, c->sp_scratch[k]);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    c->n_split = want;
    return 0;
}
// first layer of stage k of n: equal shares of the weights, the head's GEMM counting as V / (13 D) layers
uint64_t split_point(const rwkv_ctx *c, int k, int n)
{
    if (k <= 0) return 0;
    if (k >= n) return c->L;
    const double head = (double)RWKV_VOCAB / (13.0 * (double)c->D);
    uint64_t l = (uint64_t)(((double)c->L + head) * k / n + 0.5);
    if (l < (uint64_t)k) l = (uint64_t)k;                                   // every stage holds at least one layer
    if (l > c->L - (uint64_t)(n - k)) l = c->L - (uint64_t)(n - k);
    return l;
}

// The captured passes are keyed by (layer range, residual buffer, rows, logits row of the last part): a server with many different
// prompt lengths keeps adding shapes (up to max_ctx / 64 row offsets x 64 remainders for the part that holds the head).  The cache is
// bounded: beyond SQ_GRAPH_CAP entries everything is dropped and re-captured on demand (a capture costs ~1 ms per pass shape; a 512-token
// prompt uses 24).  Called at the START of rwkv_forward only (the one entry point that replays them): it is synchronous on return, so none of
// the executables is in flight here.
constexpr size_t SQ_GRAPH_CAP = 256;
void trim_pass_graphs(rwkv_ctx *c)
{
    if (c->sq_graphs.size() <= SQ_GRAPH_CAP) return;
    for (auto &kv : c->sq_graphs) (void)hipGraphExecDestroy(kv.second);
    c->sq_graphs.clear();
}

// one pass of the chunk path (GPT layout only: the key below cannot tell layouts apart): replay of the captured graph of exactly this pass shape, captured at first use.  The token
// upload stays outside (the caller's: host memory changes per pass; the pass reads the ids from its buffer's device slot); everything
// else a pass launches depends only on the key.  A capture that fails turns the graphs off for the context and the pass is launched directly.
int enqueue_pass(rwkv_ctx *c, const SeqPass &pass)
{
    if (!pass.rows.replayed()) return fail(RWKV_E_ARG, "only a GPT pass is replayed");
    if (!c->seq_graph || c->tl_on) return enqueue_chunk(c, pass);
    const rwkv_ctx::SeqGraphKey key{pass.la, pass.lb, pass.heads(c) ? pass.row0 : 0, pass.buf, pass.n};
    auto it = c->sq_graphs.find(key);
    if (it == c->sq_graphs.end()) {
        hipGraph_t g = nullptr;
        hipGraphExec_t ge = nullptr;
        bool ok = hipStreamBeginCapture(pass.st, hipStreamCaptureModeRelaxed) == hipSuccess;
        if (ok) {
            const int rc = enqueue_chunk(c, pass);
            const hipError_t e = hipStreamEndCapture(pass.st, &g);
            ok = rc == 0 && e == hipSuccess && g != nullptr;
        }
        if (ok) ok = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) == hipSuccess;
        if (g) (void)hipGraphDestroy(g);
        if (!ok) {
            (void)hipGetLastError();
            c->seq_graph = false;
            return enqueue_chunk(c, pass);
        }
        it = c->sq_graphs.emplace(key, ge).first;
    }
    HIPCHK(hipGraphLaunch(it->second, pass.st));
    return 0;
}

// rows per weight pass: 64 (two halves sharing every weight fragment) for calls of more than 32 rows, else 32
uint64_t seq_pass_rows(const rwkv_ctx *c, uint64_t T) { return (T > (uint64_t)SEQ_T && c->seq_rows > SEQ_T) ? (uint64_t)SEQ_TM : (uint64_t)SEQ_T; }

// The chunk path's schedule of T >= 2 rows (rwkv_forward's; every step of rwkv_decode_batch_* runs it too): passes of <= 64 rows and,
// for more than one pass, the software pipeline over the RWKV_SEQ_STAGES streams, in the row layout `rows` of the whole call (a
// segmented call's plan is cut for passes of seq_pass_rows(c, T): pass t0 reads plan + t0).  The token ids come from the host (`tokens`) or from
// the device array `dtok` ([T], e.g. the picks of the previous decode step) -- not for a layout that is replayed: a captured pass reads its ids
// from its buffer's slot.  Only enqueues: the context's stream holds the result when it returns.
int enqueue_rows(rwkv_ctx *c, const uint64_t *tokens, const unsigned long long *dtok, uint64_t T, const RowLayout &rows)
{
    if (dtok && rows.replayed()) return fail(RWKV_E_ARG, "a replayed pass takes its token ids from the host");
    // (the checkpoint arrays are laid out for ONE pass: enqueue_verify builds its pass itself)
    if (rows.kind == RowLayout::CKPT) return fail(RWKV_E_ARG, "a checkpointing pass is not cut into passes");
    const uint64_t CH = seq_pass_rows(c, T);
    const uint64_t nchunks = (T + CH - 1) / CH;
    int rc = 0;
    // Software pipeline over the chunks: stage k = an equal share of the layers (the last one with the head) on its
    // own stream with its own scratch, stage k on chunk i while stage k - 1 is on chunk i + 1.  Every launch of this path
    // costs ~4.5 us of start-up and tail whatever it moves; with independent kernel sequences on the GPU those run under the
    // other stages' streams (7B, 512-token prompt: 9.1k -> 12k tokens/s with three stages).  A chunk's residual stream stays
    // in its buffer (sq_x[i % ns], updated in place by every stage); results are bit-identical to the one-stream schedule, which is
    // this loop with ONE stage -- a single pass, or RWKV_SEQ_STAGES = 1: the whole layer range on the context's stream with its own
    // scratch, every pass in buffer 0, nothing to hand over and so no event (and no split_setup for a single pass: nothing is allocated).
    if (nchunks >= 2 && (rc = split_setup(c))) return rc;
    const int ns = nchunks >= 2 ? c->n_split : 1;
    for (int k = 0; rows.kind == RowLayout::SEGMENTED && k < ns; k++)      // the staging rows of the scratch sets this call uses
        if (!c->sp_scratch[k].seg && (rc = dalloc(c, &c->sp_scratch[k].seg, (size_t)SEQ_TM * c->D))) return rc;
    if (ns >= 2) HIPCHK(hipEventRecord(c->sp_end, c->stream));        // the other stages start behind whatever the context's stream holds
    for (int k = 1; k < ns; k++) HIPCHK(hipStreamWaitEvent(c->sp_stream[k], c->sp_end, 0));
    uint64_t i = 0;
    for (uint64_t t0 = 0; t0 < T && !rc; t0 += CH, i++) {
        const int n = (int)(T - t0 < CH ? T - t0 : CH);
        const int b = (int)(i % (uint64_t)ns);
        for (int k = 0; k < ns && !rc; k++) {
            hipStream_t st = c->sp_stream[k];
            if (k > 0) HIPCHK(hipStreamWaitEvent(st, c->sp_done[k - 1][b], 0));                    // the stage before has handed chunk i over
            else if (ns >= 2 && i >= (uint64_t)ns) HIPCHK(hipStreamWaitEvent(st, c->sp_done[ns - 1][b], 0));   // the last stage is done with this buffer (chunk i - ns)
            // (stage 0: the context's own stream and scratch)
            const SeqPass pass{split_point(c, k, ns), split_point(c, k + 1, ns), st, &c->sp_scratch[k], b, n, t0, dtok ? dtok + t0 : token_slot(c, b), rows.from_row(t0)};
            if (pass.embeds(c) && !dtok) rc = upload_chunk_tokens(c, tokens + t0, n, b, st);
            if (!rc) rc = pass.rows.replayed() ? enqueue_pass(c, pass) : enqueue_chunk(c, pass);
            if (ns >= 2) HIPCHK(hipEventRecord(c->sp_done[k][b], st));
        }
    }
    for (int k = 1; k < ns; k++) {                                // the context's stream owns the result again
        HIPCHK(hipEventRecord(c->sp_end, c->sp_stream[k]));
        HIPCHK(hipStreamWaitEvent(c->stream, c->sp_end, 0));
    }
    return rc;
}

// The start of every entry point, in this order: the context and the call's pointer arguments (`ptrs`) are there; the context is in the state
// the call needs; its device is current; and, for a call that launches kernels, the device error word is clear.  The word belongs to ONE call:
// an entry point that left early (a failed HIP call) never consumed it, and a code raised then would surface -- attributed to the wrong
// operation -- from whatever synchronises next.  The call's own argument checks follow behind.
enum : unsigned {
    NEED_LOADED = 1,
    NEED_WHOLE = 2,     // loaded with every layer, so with the embedding and the head too
    NEED_HEAD = 4,      // loaded as the last stage of a pipeline, or as a whole model
    NEED_SEQ = 8,       // loaded with the chunk path
    LAUNCHES = 16,
};
int guard(rwkv_ctx *c, unsigned need, bool ptrs = true)
{
    if (!c || !ptrs) return fail(RWKV_E_ARG, "NULL argument");
    if ((need & ~LAUNCHES) && !c->loaded) return fail(RWKV_E_STATE, "RWKV not loaded");                                   // rwkv.h:342-345
    if ((need & NEED_WHOLE) && (c->l0 != 0 || c->l1 != c->L)) return fail(RWKV_E_STATE, "needs a whole-model context (a pipeline stage has no embedding / head of its own)");
    if ((need & NEED_HEAD) && c->l1 != c->L) return fail(RWKV_E_STATE, "this pipeline stage does not hold the head");
    if ((need & NEED_SEQ) && !c->seq_ok) return fail(RWKV_E_STATE, "chunked path not available (load with max_ctx > 1; off with RWKV_SEQ=0 or n_embed not a multiple of 64)");
    HIPCHK(hipSetDevice(c->device));
    if ((need & LAUNCHES) && c->herr) *c->herr = 0u;
    return 0;
}

// every id of the array is one of the vocabulary's (`what`: "token" or "target")
int check_ids(const uint64_t *ids, uint64_t n, const char *what)
{
    for (uint64_t i = 0; i < n; i++)
        if (ids[i] >= RWKV_VOCAB) return fail(RWKV_E_ARG, "%s id %llu out of range", what, (unsigned long long)ids[i]);
    return 0;
}

// the token's control block (every launch of the token reads token / slot / out_row from it): staged in pinned memory, copied behind the stream's work
int set_ctl(rwkv_ctx *c, uint64_t token, unsigned slot, unsigned out_row)
{
    c->h_ctl[0].token = token; c->h_ctl[0].slot = slot; c->h_ctl[0].out_row = out_row; c->h_ctl[0].step = 0; c->h_ctl[0].pad = 0;
    HIPCHK(hipMemcpyAsync(c->ctl, &c->h_ctl[0], sizeof(Ctl), hipMemcpyHostToDevice, c->stream));
    return 0;
}

int run_token(rwkv_ctx *c, bool with_argmax)
{
    hipGraphExec_t g = with_argmax ? c->g_greedy : c->g_fwd;
    if (g) { HIPCHK(hipGraphLaunch(g, c->stream)); return 0; }
    return enqueue_token(c, with_argmax, nullptr);
}

// environment variables earlier versions read: setting one now changes nothing, so say so (replacement: nullptr = none)
const struct { const char *name, *instead; } RETIRED_ENV[] = {
    {"RWKV_RING", "RWKV_TILE (the LDS-ring form of the row-form decode kernels is gone)"},
    {"RWKV_NO_GRAPH", "RWKV_GRAPH=0"},
    {"RWKV_SEQ_GRAPH", "RWKV_GRAPH bit 1"},
    {"RWKV_SEQ_SPLIT", "RWKV_SEQ_STAGES (RWKV_SEQ_SPLIT=0 is RWKV_SEQ_STAGES=1)"},
    {"RWKV_PIPE_LOG", nullptr},
    {"RWKV_SEQ_PIPE", nullptr},
    {"RWKV_SEQ_SMALL", nullptr},
};
void warn_retired_env()
{
    for (const auto &r : RETIRED_ENV)
        if (getenv(r.name))
            fprintf(stderr, "[rwkv_mi355x] %s is retired and ignored%s%s\n", r.name, r.instead ? "; use " : "", r.instead ? r.instead : "");
}

} // namespace

extern "C" {

const char *rwkv_last_error(void) { return g_err.c_str(); }

int rwkv_create(rwkv_ctx **out, int device)
{
    if (!out) return fail(RWKV_E_ARG, "out is NULL");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(RWKV_E_DEVICE, "no HIP device available (this engine has no CPU fallback)");
    if (device < 0 || device >= n) return fail(RWKV_E_ARG, "device %d out of range (have %d)", device, n);
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    rwkv_ctx *c = new rwkv_ctx();
    c->device = device;
    c->grid = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    const char *g = getenv("RWKV_GRID");
    if (g && atoi(g) > 0) c->grid = atoi(g);
    warn_retired_env();
    { const char *e = getenv("RWKV_SEQ_B"); if (e) c->seq_b = atoi(e); }
    { const char *e = getenv("RWKV_GRAPH"); if (e) { c->graphs = atoi(e); c->seq_graph = (c->graphs & 2) != 0; } }
    { const char *e = getenv("RWKV_SEQ_ROWS"); if (e) c->seq_rows = atoi(e) > SEQ_T ? SEQ_TM : SEQ_T; }
    { const char *e = getenv("RWKV_TILE"); if (e) c->tile = atoi(e); }
    if (c->grid > NT / 2) c->grid = NT / 2;   // consumers sum one partial per thread of the prologue waves (half the workgroup)
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return fail(RWKV_E_DEVICE, "hipStreamCreate: %s", hipGetErrorString(e)); }
    void *dp = nullptr;
    if (hipHostMalloc(reinterpret_cast<void **>(&c->herr), 64, hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer(&dp, c->herr, 0) != hipSuccess) {
        if (c->herr) (void)hipHostFree(c->herr);
        (void)hipStreamDestroy(c->stream);
        delete c;
        return fail(RWKV_E_DEVICE, "cannot map the device error word");
    }
    *c->herr = 0u;
    c->d_herr = static_cast<unsigned *>(dp);
    *out = c;
    return 0;
}

int rwkv_set_layer_range(rwkv_ctx *c, uint64_t l0, uint64_t l1)
{
    if (const int rc = guard(c, 0)) return rc;
    if (c->loaded) return fail(RWKV_E_STATE, "RWKV already loaded");
    if (l0 >= l1) return fail(RWKV_E_ARG, "empty layer range");
    c->l0 = l0; c->l1 = l1;
    return 0;
}

int rwkv_load_file(rwkv_ctx *c, const char *path, uint64_t max_ctx)
{
    if (const int rc = guard(c, 0, path)) return rc;
    Source src;
    src.f = fopen(path, "rb");
    if (!src.f) return fail(RWKV_E_IO, "Error opening file %s", path);   // reference: rwkv.cu:641-645
    uint64_t hdr[2];
    if (fread(hdr, 8, 2, src.f) != 2) { fclose(src.f); return fail(RWKV_E_IO, "%s: truncated header", path); }
    uint64_t o = 16;
    for (int i = 0; i < 46; i++) { src.off[i] = o; o += tensor_elems(i, hdr[0], hdr[1]) * kTypes[i]; }
    int rc = 0;
    if (fseeko(src.f, 0, SEEK_END) != 0 || (uint64_t)ftello(src.f) < o)
        rc = fail(RWKV_E_IO, "%s: file shorter than the %llu bytes a %llu-layer, %llu-wide model needs", path,
                  (unsigned long long)o, (unsigned long long)hdr[0], (unsigned long long)hdr[1]);
    if (!rc) rc = load_common(c, src, hdr[0], hdr[1], max_ctx);
    fclose(src.f);
    return rc;
}

int rwkv_load_tensors(rwkv_ctx *c, uint64_t n_layers, uint64_t n_embed, const void *const *ptrs,
                      int on_device, uint64_t max_ctx)
{
    if (const int rc = guard(c, 0, ptrs)) return rc;
    Source src;
    src.ptrs = ptrs;
    src.on_device = on_device != 0;
    return load_common(c, src, n_layers, n_embed, max_ctx);
}

uint64_t rwkv_n_layers(const rwkv_ctx *c) { return c ? c->L : 0; }
uint64_t rwkv_n_embed(const rwkv_ctx *c) { return c ? c->D : 0; }
uint64_t rwkv_max_ctx(const rwkv_ctx *c) { return c ? c->maxT : 0; }

int rwkv_forward(rwkv_ctx *c, const uint64_t *tokens, uint64_t T, int mode)
{
    if (const int rc = guard(c, NEED_LOADED | LAUNCHES, tokens)) return rc;
    if (T > c->maxT) return fail(RWKV_E_ARG, "Context too large, max context is %llu", (unsigned long long)c->maxT);   // rwkv.h:347-350
    if (mode != RWKV_MODE_PARRALEL && mode != RWKV_MODE_GPT) return fail(RWKV_E_ARG, "bad mode %d", mode);
    if (const int rc = check_ids(tokens, T, "token")) return rc;
    trim_pass_graphs(c);
    if (T >= 2 && c->seq_ok && c->l0 == 0 && c->l1 == c->L)   // prompt chunks (GPT) / batched decode step of T streams (PARRALEL): weights read once per <= 64 rows
        return finish(c, enqueue_rows(c, tokens, nullptr, T, RowLayout::of_mode(mode)));
    return finish(c, [&]() -> int {
        for (uint64_t t = 0; t < T; t++) {
            c->h_ctl[t].token = tokens[t];
            c->h_ctl[t].slot = (mode == RWKV_MODE_PARRALEL) ? (unsigned)t : 0u;   // rwkv.cu:236-240
            c->h_ctl[t].out_row = (unsigned)t;
            c->h_ctl[t].step = 0; c->h_ctl[t].pad = 0;
            HIPCHK(hipMemcpyAsync(c->ctl, &c->h_ctl[t], sizeof(Ctl), hipMemcpyHostToDevice, c->stream));
            if (const int rc = run_token(c, false)) return rc;
        }
        return 0;
    }());
}

int rwkv_stage_forward(rwkv_ctx *c, uint64_t token, uint32_t slot, uint64_t *pick)
{
    if (const int rc = guard(c, NEED_LOADED | LAUNCHES)) return rc;
    if (slot >= c->maxT) return fail(RWKV_E_ARG, "state slot %u out of range (max context %llu)", slot, (unsigned long long)c->maxT);
    if (const int rc = check_ids(&token, c->l0 == 0, "token")) return rc;      // (a later stage takes the residual vector, not the id)
    const bool last = c->l1 == c->L;
    return finish(c, [&]() -> int {
        if (const int rc = set_ctl(c, token, slot, slot)) return rc;
        if (const int rc = run_token(c, last && pick != nullptr)) return rc;
        if (last && pick) HIPCHK(hipMemcpyAsync(pick, c->gen, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        return 0;
    }());
}

double *rwkv_x_device(rwkv_ctx *c) { return c ? c->x : nullptr; }

int rwkv_set_state(rwkv_ctx *c, const double *xy, const double *aa, const double *bb, const double *pp,
                   const double *dd, uint64_t n_slots)
{
    if (const int rc = guard(c, NEED_LOADED)) return rc;
    if (n_slots > c->maxT) return fail(RWKV_E_ARG, "n_slots %llu > max context %llu", (unsigned long long)n_slots, (unsigned long long)c->maxT);
    const double *h[5] = {xy, aa, bb, pp, dd};
    const size_t bytes = n_slots * c->L * c->D * sizeof(double);
    return finish(c, [&]() -> int {
        for (int s = 0; s < 5; s++)
            if (h[s]) HIPCHK(hipMemcpyAsync(c->state[s], h[s], bytes, hipMemcpyHostToDevice, c->stream));
        return 0;
    }());
}

int rwkv_get_output(rwkv_ctx *c, float *logits, double *xy, double *aa, double *bb, double *pp, double *dd,
                    uint64_t T)
{
    if (const int rc = guard(c, NEED_LOADED)) return rc;
    if (T > c->maxT) return fail(RWKV_E_ARG, "n_tokens %llu > max context %llu", (unsigned long long)T, (unsigned long long)c->maxT);
    double *h[5] = {xy, aa, bb, pp, dd};
    const size_t bytes = T * c->L * c->D * sizeof(double);
    return finish(c, [&]() -> int {
        if (logits) HIPCHK(hipMemcpyAsync(logits, c->logits, T * RWKV_VOCAB * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        for (int s = 0; s < 5; s++)
            if (h[s]) HIPCHK(hipMemcpyAsync(h[s], c->state[s], bytes, hipMemcpyDeviceToHost, c->stream));
        return 0;
    }());
}

namespace {
int enqueue_reset(rwkv_ctx *c)
{
    for (int s = 0; s < 5; s++)
        HIPCHK(hipMemsetAsync(c->state[s], 0, c->maxT * c->L * c->D * sizeof(double), c->stream));
    return 0;
}

// ---- stop sequences and budgets (stop.hip.h): the stop test of a generation call (DecodeRun, below) ----
// One call's stopping, set up by stopper_setup.  after_step is the last part of a step and says whether another one follows; unpark belongs to the
// call's end.  The run-ahead is bounded, not drained: the active count of block b (RWKV_STOP_POLL steps) travels into word b % STOP_RING of the
// pinned ring behind the block, and block b + 2 is enqueued only after that word has arrived non-zero.
struct Stopper {
    StopArgs a{};
    ParkArgs p{};
    uint64_t steps_run = 0;
    // step k has been picked into picks[0 .. n); more: enqueue the next step
    int after_step(rwkv_ctx *c, uint64_t k, const unsigned long long *picks, bool *more)
    {
        k_stop_step<<<dim3((a.n + STOP_NT - 1) / STOP_NT), dim3(STOP_NT), 0, c->stream>>>(a, picks, (unsigned)k);
        k_stop_park<false><<<dim3(PARK_CHUNKS, a.n), dim3(PARK_NT), 0, c->stream>>>(p, (unsigned)k + 1);
        HIPCHK(hipGetLastError());
        steps_run = k + 1;
        *more = true;
        if (steps_run % RWKV_STOP_POLL) return 0;
        const uint64_t b = steps_run / RWKV_STOP_POLL - 1;          // the block that ends here
        HIPCHK(hipMemcpyAsync(&c->stop_ring[b % rwkv_ctx::STOP_RING], a.active, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipEventRecord(c->stop_ev[b % rwkv_ctx::STOP_RING], c->stream));
        if (b >= 1) {                                               // block b + 1 >= 2 is next: it waits for block b - 1
            HIPCHK(hipEventSynchronize(c->stop_ev[(b - 1) % rwkv_ctx::STOP_RING]));
            *more = c->stop_ring[(b - 1) % rwkv_ctx::STOP_RING] != 0ull;
        }
        return 0;
    }
    // behind the last enqueued step: every stopped stream gets back what it held when it stopped
    int unpark(rwkv_ctx *c)
    {
        k_stop_park<true><<<dim3(PARK_CHUNKS, a.n), dim3(PARK_NT), 0, c->stream>>>(p, 0u);
        HIPCHK(hipGetLastError());
        return 0;
    }
};

// ---- log-probs and top-n alternatives of the picks (topn.hip.h): the record of a generation call ----
// LP_REC in 8-byte words for R rows per step, S steps and top-n n: where the score tuples, the candidates and step 0 of the record start, the words of
// one step (logprob [R] | entropy [R] | top ids [R][n] | top logprob [R][n]) and of the whole buffer
struct LpLayout {
    size_t part, cand, rec, step, words;
    LpLayout(uint64_t R, uint64_t S, uint64_t n) : part(R), cand(part + R * SC_PART_Q), rec(cand + R * SC_G * n), step(R * (2 + 2 * n)), words(rec + S * step) {}
};
// One call's record, set up by lp_setup.  record is the part of a step between the pick and the stop test: two launches over rows 0 .. R - 1
// that read the logits rows and the picks and write step k of the record, nothing else.
struct LpRecorder {
    TopnArgs a{};
    double *rec = nullptr;
    size_t step = 0;
    unsigned R = 0;
    static int launch(rwkv_ctx *c, const TopnArgs &t, unsigned rows)
    {
        k_topn_part<<<dim3(SC_G, rows), dim3(SC_NT), 0, c->stream>>>(t);
        k_topn_finish<<<dim3(rows), dim3(std::max(64u, (SC_G * t.n + 63u) / 64u * 64u)), 0, c->stream>>>(t);
        HIPCHK(hipGetLastError());
        return 0;
    }
    int record(rwkv_ctx *c, uint64_t k, const unsigned long long *picks) const
    {
        TopnArgs t = a;
        double *base = rec + k * step;
        t.picks = picks; t.pick_logprob = base; t.entropy = base + R;
        t.ids = reinterpret_cast<unsigned long long *>(base + 2 * (size_t)R); t.logprob = base + (2 + (size_t)t.n) * R;
        return launch(c, t, R);
    }
};

// ---- how a call picks its tokens: rwkv_pick, the C ABI's record, is the internal description too (sampler.hip.h, nucleus.hip.h) ----
static_assert(sizeof(rwkv_nucleus_params) == 32, "rwkv_nucleus_params is 32 bytes in the C ABI");
rwkv_pick pick_greedy() { rwkv_pick pk{}; pk.kind = RWKV_PICK_GREEDY; return pk; }
rwkv_pick pick_typical(float temp, float tau, int flags) { rwkv_pick pk{}; pk.kind = RWKV_PICK_TYPICAL; pk.temp = temp; pk.tau = tau; pk.typical_flags = flags; return pk; }
rwkv_pick pick_nucleus(const rwkv_nucleus_params &np) { rwkv_pick pk{}; pk.kind = RWKV_PICK_NUCLEUS; pk.nucleus = np; return pk; }
constexpr uint32_t NUCLEUS_FLAGS = RWKV_NUCLEUS_BAN0 | RWKV_NUCLEUS_KEEP | RWKV_NUCLEUS_UPDATE;
int check_nucleus(const rwkv_nucleus_params *p)
{
    if (!(p->temp > 0.f)) return fail(RWKV_E_ARG, "need temp > 0");
    if (!std::isfinite(p->top_p) || !std::isfinite(p->presence) || !std::isfinite(p->frequency)) return fail(RWKV_E_ARG, "top_p, presence and frequency must be finite");
    if (!(p->decay >= 0.f && p->decay <= 1.f)) return fail(RWKV_E_ARG, "decay must be in [0, 1]");
    if ((p->flags & ~NUCLEUS_FLAGS) || p->reserved) return fail(RWKV_E_ARG, "unknown flag bits (0x%x) or reserved != 0", p->flags);
    return 0;
}
// the pick's own parameters are acceptable
int check_pick(const rwkv_pick &pk)
{
    switch (pk.kind) {
    case RWKV_PICK_GREEDY: return 0;
    case RWKV_PICK_TYPICAL: return pk.temp > 0.f ? 0 : fail(RWKV_E_ARG, "need temp > 0");
    case RWKV_PICK_NUCLEUS: return check_nucleus(&pk.nucleus);
    default: return fail(RWKV_E_ARG, "unknown pick kind %d", pk.kind);
    }
}
// an unknown kind answers in front of decode_batch's checks
int check_pick_kind(const rwkv_pick &pk) { return pk.kind < RWKV_PICK_GREEDY || pk.kind > RWKV_PICK_NUCLEUS ? check_pick(pk) : 0; }
// the ranges that several entry points share, each in the caller's words
int check_steps(uint64_t n, const char *name) { return n == 0 || n > RWKV_MAX_DECODE_STEPS ? fail(RWKV_E_ARG, "%s must be in 1..%u", name, RWKV_MAX_DECODE_STEPS) : 0; }
int check_row_slot(const rwkv_ctx *c, uint64_t row, uint64_t slot)
{
    return row < c->maxT && slot < c->maxT ? 0 : fail(RWKV_E_ARG, "logits row %llu or slot %llu out of range (max context %llu)", (unsigned long long)row, (unsigned long long)slot, (unsigned long long)c->maxT);
}
int check_slot_span(const rwkv_ctx *c, uint64_t slot0, uint64_t n)
{
    return n != 0 && slot0 < c->maxT && n <= c->maxT - slot0 ? 0 : fail(RWKV_E_ARG, "slots %llu .. + %llu out of range (max context %llu)", (unsigned long long)slot0, (unsigned long long)n, (unsigned long long)c->maxT);
}
bool pick_penalty(const rwkv_pick &pk) { return pk.kind == RWKV_PICK_NUCLEUS && (pk.nucleus.presence != 0.f || pk.nucleus.frequency != 0.f); }
// the count vectors (device [max_ctx][V] f32): allocated and zeroed once
int counts_alloc(rwkv_ctx *c)
{
    if (c->grown[PEN_COUNTS].p) return 0;
    const size_t bytes = sizeof(float) * c->maxT * RWKV_VOCAB;
    void *q = nullptr;
    HIPCHK(hipMalloc(&q, bytes));
    c->grown[PEN_COUNTS].p = q; c->grown[PEN_COUNTS].bytes = bytes; c->alloc_bytes += bytes;
    HIPCHK(hipMemsetAsync(q, 0, bytes, c->stream));
    return 0;
}
// what a call with this pick needs of the counts of slots [slot0, slot0 + n): nothing without a penalty; else the buffer, and (`zero`: the
// loops) those vectors cleared unless the caller keeps them
int pick_counts(rwkv_ctx *c, const rwkv_pick &pk, uint64_t slot0, uint64_t n, bool zero)
{
    if (!pick_penalty(pk)) return 0;
    const bool fresh = !c->grown[PEN_COUNTS].p;
    if (const int rc = counts_alloc(c)) return rc;
    if (zero && !fresh && !(pk.nucleus.flags & RWKV_NUCLEUS_KEEP))
        HIPCHK(hipMemsetAsync(c->buf<float>(PEN_COUNTS) + slot0 * RWKV_VOCAB, 0, sizeof(float) * n * RWKV_VOCAB, c->stream));
    return 0;
}

// One call's sampler: the kind (RWKV_PICK_TYPICAL or _NUCLEUS) and that kind's kernel arguments
struct Sampler {
    int kind = RWKV_PICK_GREEDY;
    TypicalArgs t{};
    NucleusArgs n{};
    DrawArgs &draw() { return kind == RWKV_PICK_NUCLEUS ? static_cast<DrawArgs &>(n) : t; }
};
// The sampler of a call that picks by `pk` (not greedy), on the context's single-row scratch.  `loop`: as a generation call of one stream runs it
// (logit 0 always banned, the counts always updated, row and step from the control block, u from seed + step, the pick fed back); else the
// caller sets row and u.  Call behind pick_counts.
Sampler make_sampler(rwkv_ctx *c, const rwkv_pick &pk, bool loop)
{
    Sampler s;
    s.kind = pk.kind;
    DrawArgs &d = s.draw();
    d.logits = c->logits; d.ctl = c->ctl; d.gen = c->gen; d.gen_cap = c->gen_cap;
    d.step = -1; d.seeds = nullptr;
    d.pick = c->pick; d.part = c->ts_part; d.p = c->ts_p; d.pw = c->ts_pw; d.key = c->ts_key;
    if (loop) { d.row = -1; d.use_seed = 1; d.feedback = 1; }
    if (pk.kind == RWKV_PICK_TYPICAL) {
        // default: what typical.h computes -- no cut (typical.h:50 assigns into a temporary), integer exponent
        // uint8(1/temp) (nc::power, typical.h:52); RWKV_SAMPLE_RECIPE: the documented recipe
        s.t.recipe = (pk.typical_flags & RWKV_SAMPLE_RECIPE) ? 1 : 0;
        if (s.t.recipe) s.t.expo = pk.temp == 1.0f ? 1.0 : 1.0 / (double)pk.temp;
        else { const double e = 1.0 / (double)pk.temp; s.t.expo = pk.temp == 1.0f ? 1.0 : (e >= 255.0 ? 255.0 : (double)(unsigned char)e); }
        s.t.tau = pk.tau;
        d.ban0 = (loop || (pk.typical_flags & RWKV_SAMPLE_BAN0)) ? 1 : 0;
    } else {
        const rwkv_nucleus_params &p = pk.nucleus;
        s.n.inv_temp = p.temp == 1.0f ? 1.0 : 1.0 / (double)p.temp;
        s.n.top_p = p.top_p; s.n.top_k = p.top_k >= RWKV_VOCAB ? 0u : p.top_k;
        s.n.presence = p.presence; s.n.frequency = p.frequency; s.n.decay = p.decay;
        s.n.penalty = pick_penalty(pk) ? 1 : 0;
        s.n.update = (loop || (p.flags & RWKV_NUCLEUS_UPDATE)) ? 1 : 0;
        d.ban0 = (loop || (p.flags & RWKV_NUCLEUS_BAN0)) ? 1 : 0;
        s.n.counts = s.n.penalty ? c->buf<float>(PEN_COUNTS) : nullptr;
    }
    return s;
}
// the form of it in a generation call of many streams: rows 0 .. N - 1 (slots 0 .. N - 1) with a scratch slice and a seed each, the picks not fed back
void sampler_to_batch(rwkv_ctx *c, Sampler &s, const unsigned long long *dseeds)
{
    DrawArgs &d = s.draw();
    d.row = 0; d.use_seed = 1; d.seeds = dseeds; d.feedback = 0;
    d.part = c->buf<double>(BD_PART); d.p = c->buf<float>(BD_P);
    d.pw = c->buf<float>(BD_PW); d.key = c->buf<unsigned>(BD_KEY);
}
// the sampler's three launches over `rows` logits rows (row onwards), each row with its own scratch slice and pick
int enqueue_pick(rwkv_ctx *c, const Sampler &s, unsigned rows)
{
    if (s.kind == RWKV_PICK_NUCLEUS) {
        k_nucleus_stats<<<dim3(TS_G, rows), dim3(TS_GT), 0, c->stream>>>(s.n);
        k_nucleus_keys<<<dim3(TS_G, rows), dim3(TS_GT), 0, c->stream>>>(s.n);
        k_nucleus<<<dim3(1, rows), dim3(TS_NT), 0, c->stream>>>(s.n);
    } else {
        k_typical_stats<<<dim3(TS_G, rows), dim3(TS_GT), 0, c->stream>>>(s.t);
        k_typical_keys<<<dim3(TS_G, rows), dim3(TS_GT), 0, c->stream>>>(s.t);
        k_typical<<<dim3(1, rows), dim3(TS_NT), 0, c->stream>>>(s.t);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// the row pick of the greedy kind: k_argmax_rows and its finish over n rows from `base` on, the ids into `ids` (BD_VAL / BD_IDX hold the partials)
int enqueue_argmax_rows(rwkv_ctx *c, const float *base, unsigned n, unsigned long long *ids)
{
    float *val = c->buf<float>(BD_VAL);
    unsigned *idx = c->buf<unsigned>(BD_IDX);
    k_argmax_rows<<<dim3(AM_SLICES, n), dim3(AM_NT), 0, c->stream>>>(base, val, idx);
    k_argmax_rows_finish<<<dim3(n), dim3(64), 0, c->stream>>>(val, idx, ids);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- constrained decoding (constrain.hip.h): the constraint of a generation call, or of one rwkv_pick_constrained ----
// One call's constraint, set up by constrainer_setup.  rows() writes the constrained rows into the second buffer, the pick reads them there (a
// sampler after feed(), the greedy kind as enqueue_argmax_rows over that buffer), advance() moves the automaton states behind the pick.
struct Constrainer {
    ConstrainArgs r{};
    AdvanceArgs v{};
    int rows(rwkv_ctx *c, unsigned n) const
    {
        k_constrain_rows<0><<<dim3(CN_SLICES, n), dim3(CN_NT), 0, c->stream>>>(r);
        HIPCHK(hipGetLastError());
        return 0;
    }
    // the sampler reads the constrained rows and bans nothing itself: they already hold -inf at id 0
    void feed(Sampler &s) const { s.draw().logits = r.out; s.draw().ban0 = 0; }
    int advance(rwkv_ctx *c, const unsigned long long *picks) const
    {
        k_constraint_advance<0><<<dim3((v.n + CN_ADV_NT - 1) / CN_ADV_NT), dim3(CN_ADV_NT), 0, c->stream>>>(v, picks);
        HIPCHK(hipGetLastError());
        return 0;
    }
};

// ---- a generation call: what it is (here), and how it runs (DecodeRun, below the setup functions of its parts) ----
// rwkv_decode_greedy / _typical / _nucleus and rwkv_decode_batch_greedy / _typical / _nucleus / _until / _logprobs / _constrained fill this and hand
// it on.  A null member means that the part is absent (trailing members left out of the initialiser are null).
struct DecodeCall {
    uint64_t N, n_steps;                            // streams (on slots 0 .. N - 1) and steps
    const uint64_t *first, *seeds;                  // [N] each; the seeds of a sampled pick
    rwkv_pick pick;
    uint64_t *out_tokens;                           // [N][n_steps]
    const rwkv_stop_params *stop;                   // stop sequences and budgets
    uint32_t *out_len, *out_reason;                 // [N] each
    uint64_t *steps_run;
    const rwkv_logprob_out *lp;                     // the record, with the caller's arrays for it
    const rwkv_constrain_params *cp;                // the constraint, with the caller's out_state
};
int run_call(rwkv_ctx *c, const DecodeCall &d, const StopTable *table = nullptr);
// the checks of rwkv_decode_greedy / _typical / _nucleus behind the guard: one stream on slot 0
int decode_one(rwkv_ctx *c, uint64_t first_token, uint64_t n, const rwkv_pick &pk, uint64_t seed, uint64_t *out_tokens)
{
    if (const int rc = check_ids(&first_token, 1, "token")) return rc;
    if (n == 0 || n > c->gen_cap) return fail(RWKV_E_ARG, "n_tokens must be in 1..%u", c->gen_cap);
    if (const int rc = check_pick(pk)) return rc;
    return run_call(c, DecodeCall{1, n, &first_token, &seed, pk, out_tokens});
}
} // namespace

int rwkv_reset_state(rwkv_ctx *c)
{
    if (const int rc = guard(c, NEED_LOADED)) return rc;
    return finish(c, enqueue_reset(c));
}

int rwkv_decode_greedy(rwkv_ctx *c, uint64_t first_token, uint64_t n, uint64_t *out_tokens)
{
    if (const int rc = guard(c, NEED_WHOLE | LAUNCHES, out_tokens)) return rc;
    return decode_one(c, first_token, n, pick_greedy(), 0, out_tokens);
}

int rwkv_sample_typical(rwkv_ctx *c, uint64_t row, float temp, float tau, double u, int flags, uint64_t *token)
{
    if (const int rc = guard(c, NEED_HEAD | LAUNCHES, token)) return rc;
    if (row >= c->maxT) return fail(RWKV_E_ARG, "logits row %llu out of range (max context %llu)", (unsigned long long)row, (unsigned long long)c->maxT);
    if (!(temp > 0.f) || !(u >= 0.0 && u < 1.0)) return fail(RWKV_E_ARG, "need temp > 0 and 0 <= u < 1");
    Sampler s = make_sampler(c, pick_typical(temp, tau, flags), false);
    s.t.row = (int)row; s.t.u = u;
    return finish(c, [&]() -> int {
        if (const int rc = enqueue_pick(c, s, 1)) return rc;
        HIPCHK(hipMemcpyAsync(token, c->pick, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        return 0;
    }());
}

int rwkv_decode_typical(rwkv_ctx *c, uint64_t first_token, uint64_t n, float temp, float tau, uint64_t seed, int flags, uint64_t *out_tokens)
{
    if (const int rc = guard(c, NEED_WHOLE | LAUNCHES, out_tokens)) return rc;
    return decode_one(c, first_token, n, pick_typical(temp, tau, flags), seed, out_tokens);
}

namespace {
// grow one of the context's buffers to `bytes` (contents are not kept); counted in rwkv_resident_bytes
int grow_buffer(rwkv_ctx *c, GrownBuf which, size_t bytes)
{
    rwkv_ctx::Grown &g = c->grown[which];
    if (bytes <= g.bytes) return 0;
    if (g.p) {
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipFree(g.p));
        c->alloc_bytes -= g.bytes;
        g.p = nullptr; g.bytes = 0;
    }
    HIPCHK(hipMalloc(&g.p, bytes));
    g.bytes = bytes; c->alloc_bytes += bytes;
    return 0;
}

// ---- the host side of stopping (rwkv_decode_batch_until, rwkv_debug_stop_scan) ----
static_assert(sizeof(rwkv_pick) == 48 && sizeof(rwkv_stop_params) == 40, "rwkv_pick is 48 bytes and rwkv_stop_params 40 in the C ABI");
static_assert(STOP_MAX_SEQS == RWKV_STOP_MAX_SEQS && STOP_MAX_LEN == RWKV_STOP_MAX_LEN, "stop.hip.h holds the header's limits");
// the stop parameters of a call over N streams and n_steps steps are acceptable; t: the sequences as the kernels read them (newest id first)
int check_stop(const rwkv_stop_params *sp, uint64_t N, uint64_t n_steps, StopTable *t)
{
    if ((sp->flags & ~RWKV_STOP_KEEP) || sp->reserved) return fail(RWKV_E_ARG, "unknown stop flag bits (0x%x) or reserved != 0", sp->flags);
    if (sp->n_seqs > RWKV_STOP_MAX_SEQS) return fail(RWKV_E_ARG, "at most %u stop sequences", RWKV_STOP_MAX_SEQS);
    if (sp->n_seqs && (!sp->seq_ids || !sp->seq_len)) return fail(RWKV_E_ARG, "NULL argument");
    t->n_seqs = sp->n_seqs;
    const uint64_t *ids = sp->seq_ids;
    for (uint32_t j = 0; j < sp->n_seqs; ids += sp->seq_len[j++]) {
        const uint32_t len = sp->seq_len[j];
        if (len == 0 || len > RWKV_STOP_MAX_LEN) return fail(RWKV_E_ARG, "stop sequence %u: length %u is not in 1..%u", j, len, RWKV_STOP_MAX_LEN);
        if (const int rc = check_ids(ids, len, "stop")) return rc;
        t->len[j] = len;
        for (uint32_t i = 0; i < len; i++) t->ids[j][i] = (unsigned)ids[len - 1 - i];
    }
    for (uint64_t s = 0; sp->max_new && s < N; s++)
        if (sp->max_new[s] == 0 || sp->max_new[s] > n_steps) return fail(RWKV_E_ARG, "max_new[%llu] = %u is not in 1..n_steps", (unsigned long long)s, sp->max_new[s]);
    return 0;
}

// The run record of N streams (STOP_RUN on the device, stop_host its image), in 32-bit words: active (2) | first [N] (2 each) | len [N] | reason [N] |
// max_new [N].  Where len starts (reason and max_new follow it at N and 2 N) and the record's size
constexpr size_t stop_run_len(uint64_t N) { return 2 + 2 * N; }
constexpr size_t stop_run_words(uint64_t N) { return stop_run_len(N) + 3 * N; }
// the buffers and the upload of one call's stopping (sp == nullptr: no sequence, no budget, no flag -- only its automaton ends a stream): the run
// record (STOP_RUN), the histories (once), and -- `park`: a generation call, not the planted scan -- the park buffer, the poll ring and, with
// `penalty`, the count vectors that are parked with the state
int stopper_setup(rwkv_ctx *c, Stopper &st, const StopTable &t, const rwkv_stop_params *sp, const uint64_t *first, uint64_t N, uint64_t n_steps,
                  bool park, bool penalty)
{
    if (park && !c->stop_ring) {
        HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&c->stop_ring), sizeof(unsigned long long) * rwkv_ctx::STOP_RING, hipHostMallocDefault));
        for (auto &e : c->stop_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    if (!c->grown[STOP_HISTORY].p) {
        if (const int rc = grow_buffer(c, STOP_HISTORY, sizeof(unsigned) * c->maxT * STOP_HIST)) return rc;
        HIPCHK(hipMemsetAsync(c->grown[STOP_HISTORY].p, 0xFF, sizeof(unsigned) * c->maxT * STOP_HIST, c->stream));      // STOP_NONE everywhere
    }
    if (const int rc = grow_buffer(c, STOP_RUN, sizeof(unsigned) * stop_run_words(N))) return rc;
    const size_t LD = (size_t)c->L * c->D, stride = 10 * LD + PARK_ROW * (penalty ? 2 : 1);
    if (const int rc = park ? grow_buffer(c, STOP_PARK, sizeof(float) * stride * N) : 0) return rc;
    if (const int rc = park && penalty ? counts_alloc(c) : 0) return rc;
    // host image of STOP_RUN (stop_run_len, stop_run_words): active | first [N] | len [N] = 0 | reason [N] = 0 | max_new [N]
    c->stop_host.assign(stop_run_words(N), 0u);
    const unsigned long long active = N;
    memcpy(&c->stop_host[0], &active, 8);
    memcpy(&c->stop_host[2], first, 8 * N);
    for (uint64_t s = 0; s < N; s++) c->stop_host[stop_run_len(N) + 2 * N + s] = sp && sp->max_new ? sp->max_new[s] : (unsigned)n_steps;
    unsigned *run = c->buf<unsigned>(STOP_RUN);
    HIPCHK(hipMemcpyAsync(run, c->stop_host.data(), sizeof(unsigned) * stop_run_words(N), hipMemcpyHostToDevice, c->stream));
    st.a.t = t; st.a.n = (unsigned)N; st.a.n_steps = (unsigned)n_steps; st.a.keep = sp && (sp->flags & RWKV_STOP_KEEP) ? 1 : 0;
    st.a.hist = c->buf<unsigned>(STOP_HISTORY);
    st.a.active = reinterpret_cast<unsigned long long *>(run);
    st.a.first = st.a.active + 1;
    st.a.len = run + stop_run_len(N); st.a.reason = st.a.len + N; st.a.max_new = st.a.reason + N;
    for (int i = 0; i < 5; i++) st.p.state[i] = c->state[i];
    st.p.logits = c->logits; st.p.counts = penalty ? c->buf<float>(PEN_COUNTS) : nullptr;
    st.p.park = c->buf<float>(STOP_PARK); st.p.LD = LD; st.p.stride = stride; st.p.len = st.a.len;
    return 0;
}
// behind the call's last launch: lengths and reasons come back into the host image
int stopper_download(rwkv_ctx *c, const Stopper &st)
{
    HIPCHK(hipMemcpyAsync(&c->stop_host[stop_run_len(st.a.n)], st.a.len, sizeof(unsigned) * 2 * st.a.n, hipMemcpyDeviceToHost, c->stream));
    return 0;
}
// behind the wait: the call's lengths (a stream that never stopped: all n_steps) and reasons out of the host image, into those of the two arrays
// that the caller gave; `stopped` false: the call could stop no stream and has no image
void stop_results(const rwkv_ctx *c, bool stopped, uint64_t N, uint64_t n_steps, uint32_t *out_len, uint32_t *out_reason)
{
    for (uint64_t s = 0; s < N; s++) {
        const unsigned len = stopped ? c->stop_host[stop_run_len(N) + s] : 0u, reason = stopped ? c->stop_host[stop_run_len(N) + N + s] : 0u;
        if (out_len) out_len[s] = len ? len : (uint32_t)n_steps;
        if (out_reason) out_reason[s] = reason;
    }
}

// the record of a call over R rows per step (rows 0 .. R - 1: rows == nullptr) and S steps: LP_REC, and the kernels' arguments
int lp_setup(rwkv_ctx *c, LpRecorder &r, uint64_t R, uint64_t S, uint32_t top_n)
{
    const LpLayout lay(R, S, top_n);
    if (const int rc = grow_buffer(c, LP_REC, sizeof(double) * lay.words)) return rc;
    unsigned long long *w = c->buf<unsigned long long>(LP_REC);
    r.a.logits = c->logits; r.a.rows = nullptr; r.a.picks = nullptr;
    r.a.part = reinterpret_cast<double *>(w + lay.part); r.a.cand = w + lay.cand; r.a.n = top_n;
    r.rec = reinterpret_cast<double *>(w + lay.rec); r.step = lay.step; r.R = (unsigned)R;
    return 0;
}
// the one download of the record: the steps that ran
int lp_download(rwkv_ctx *c, const LpRecorder &r, uint64_t ran)
{
    c->lp_host.resize(ran * r.step);
    HIPCHK(hipMemcpyAsync(c->lp_host.data(), r.rec, sizeof(double) * ran * r.step, hipMemcpyDeviceToHost, c->stream));
    return 0;
}
// behind the wait: [step][stream] -> [stream][step] into the caller's arrays; 0 / 0.0 from a stream's end on (len == nullptr: no stream ended)
void lp_results(const rwkv_ctx *c, const rwkv_logprob_out &o, uint64_t N, uint64_t n_steps, const uint32_t *len)
{
    const uint64_t n = o.top_n, step = N * (2 + 2 * n);
    for (uint64_t s = 0; s < N; s++)
        for (uint64_t k = 0; k < n_steps; k++) {
            const bool on = !len || k < len[s];
            const unsigned long long *h = on ? c->lp_host.data() + k * step : nullptr;
            const size_t at = s * n_steps + k;
            if (on) memcpy(&o.logprob[at], h + s, 8); else o.logprob[at] = 0.0;
            if (o.entropy) { if (on) memcpy(&o.entropy[at], h + N + s, 8); else o.entropy[at] = 0.0; }
            for (uint64_t j = 0; j < n; j++) {
                o.top_ids[at * n + j] = on ? h[2 * N + s * n + j] : 0ull;
                if (on) memcpy(&o.top_logprob[at * n + j], h + (2 + n) * N + s * n + j, 8); else o.top_logprob[at * n + j] = 0.0;
            }
        }
}

// ---- the host side of constrained decoding (rwkv_constraint_*, rwkv_pick_constrained, rwkv_decode_batch_constrained) ----
static_assert(sizeof(rwkv_automaton) == 40 && sizeof(rwkv_bias) == 24 && sizeof(rwkv_constrain_params) == 48, "the constraint records of the C ABI");
static_assert(CN_MAX_STATES == RWKV_CONSTRAINT_MAX_STATES && CN_MAX_BIAS == RWKV_CONSTRAINT_MAX_BIAS && CN_STOP_REASON == RWKV_STOP_CONSTRAINT &&
              STOP_CONSTRAINT == RWKV_STOP_CONSTRAINT, "constrain.hip.h and stop.hip.h hold the header's limits");
// the host copy of the slots' automaton states (all 0 until something writes them): no device work
std::vector<unsigned> &cn_states(rwkv_ctx *c)
{
    if (c->cn_q.size() != c->maxT) c->cn_q.assign(c->maxT, 0u);
    return c->cn_q;
}
bool cn_terminal(const rwkv_ctx *c, unsigned q) { return c->cn_row_ptr[q] == c->cn_row_ptr[q + 1]; }
// a bias list is acceptable (include/rwkv_sampler.h constraint_check, the one validator)
int check_bias(uint64_t n, const uint32_t *tok, const float *val)
{
    const bias_view b{n, tok, val};
    if (const char *rule = constraint_check(nullptr, &b)) return fail(RWKV_E_ARG, "malformed bias list: %s", rule);
    return 0;
}
// slot `slot` may start a constrained pick in state q
int check_start(const rwkv_ctx *c, uint64_t slot, unsigned q)
{
    if (!c->cn_S) return q == 0u ? 0 : fail(RWKV_E_ARG, "slot %llu: automaton state %u without an installed automaton", (unsigned long long)slot, q);
    if (q >= c->cn_S) return fail(RWKV_E_ARG, "slot %llu: automaton state %u is not below %u", (unsigned long long)slot, q, c->cn_S);
    if (cn_terminal(c, q)) return fail(RWKV_E_ARG, "slot %llu: automaton state %u is terminal: nothing may follow", (unsigned long long)slot, q);
    return 0;
}
// the constraint of a call over N streams is acceptable
int check_constrain(rwkv_ctx *c, const rwkv_constrain_params &cp, const rwkv_pick &pk, uint64_t N)
{
    if (cp.reserved) return fail(RWKV_E_ARG, "reserved != 0");
    if (pk.kind == RWKV_PICK_TYPICAL) return fail(RWKV_E_ARG, "typical sampling under a constraint is out of scope: pick greedy or nucleus");
    if ((cp.bias_ptr != nullptr) != (cp.bias_tok != nullptr) || (cp.bias_ptr != nullptr) != (cp.bias_val != nullptr))
        return fail(RWKV_E_ARG, "bias_ptr, bias_tok and bias_val are all NULL or none");
    if (cp.bias_ptr && cp.bias_ptr[0] != 0u) return fail(RWKV_E_ARG, "malformed bias list: bias_ptr[0] != 0");
    for (uint64_t s = 0; cp.bias_ptr && s < N; s++) {
        if (cp.bias_ptr[s + 1] < cp.bias_ptr[s]) return fail(RWKV_E_ARG, "malformed bias list: bias_ptr decreases at stream %llu", (unsigned long long)s);
        if (const int rc = check_bias(cp.bias_ptr[s + 1] - cp.bias_ptr[s], cp.bias_tok + cp.bias_ptr[s], cp.bias_val + cp.bias_ptr[s])) return rc;
    }
    const std::vector<unsigned> &q = cn_states(c);
    for (uint64_t s = 0; s < N; s++)
        if (const int rc = check_start(c, s, cp.start ? cp.start[s] : q[s])) return rc;
    return 0;
}
// what every constrained pick needs on the device: the second row buffer, the slots' states and, without an automaton, the implicit state's mask
int constraint_buffers(rwkv_ctx *c)
{
    if (const int rc = grow_buffer(c, CN_ROWS, sizeof(float) * c->maxT * RWKV_VOCAB)) return rc;
    if (!c->grown[CN_Q].p) {
        if (const int rc = grow_buffer(c, CN_Q, sizeof(unsigned) * c->maxT)) return rc;
        HIPCHK(hipMemsetAsync(c->grown[CN_Q].p, 0, sizeof(unsigned) * c->maxT, c->stream));
    }
    if (!c->cn_S && !c->grown[CN_MASK1].p) {
        if (const int rc = grow_buffer(c, CN_MASK1, sizeof(unsigned) * CN_WORDS)) return rc;
        k_constraint_mask<0><<<dim3(1), dim3(CN_NT), 0, c->stream>>>(CsrArgs{nullptr, nullptr, nullptr, 1u}, c->buf<unsigned>(CN_MASK1));
        HIPCHK(hipGetLastError());
    }
    return 0;
}
CsrArgs csr_args(const rwkv_ctx *c)
{
    const unsigned *w = c->buf<unsigned>(CN_CSR);
    if (!c->cn_S) return CsrArgs{nullptr, nullptr, nullptr, 0u};
    return CsrArgs{w, w + c->cn_S + 1, w + c->cn_S + 1 + c->cn_nnz, c->cn_S};
}
// The buffers and the one upload of a constrained pick over n rows: rows row0 .. row0 + n - 1 with slots slot0 .. slot0 + n - 1, the bias lists
// (bias_ptr [n + 1] into tok / val; nullptr: none) as CN_CALL: bias_ptr | tok | val | done [n] (`done` with a stopper `st` only: it reads the words).
// start: the states a generation call starts its slots in go up too (host copy first: it is what the checks read); nullptr: where they stand
int constrainer_setup(rwkv_ctx *c, Constrainer &cn, uint64_t row0, uint64_t slot0, uint64_t n, const uint32_t *bias_ptr, const uint32_t *bias_tok,
                      const float *bias_val, Stopper *st, const uint32_t *start = nullptr)
{
    if (const int rc = constraint_buffers(c)) return rc;
    const size_t nb = bias_ptr ? bias_ptr[n] : 0, words = n + 1 + 2 * nb;
    if (const int rc = grow_buffer(c, CN_CALL, sizeof(unsigned) * (words + n))) return rc;
    unsigned *call = c->buf<unsigned>(CN_CALL);
    if (bias_ptr) {
        c->cn_host.assign(words, 0u);
        memcpy(c->cn_host.data(), bias_ptr, sizeof(unsigned) * (n + 1));
        if (nb) { memcpy(c->cn_host.data() + n + 1, bias_tok, sizeof(unsigned) * nb); memcpy(c->cn_host.data() + n + 1 + nb, bias_val, sizeof(float) * nb); }
        HIPCHK(hipMemcpyAsync(call, c->cn_host.data(), sizeof(unsigned) * words, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(hipMemsetAsync(call + words, 0, sizeof(unsigned) * n, c->stream));
    cn.r.logits = c->logits; cn.r.out = c->buf<float>(CN_ROWS); cn.r.row = (int)row0; cn.r.ctl = c->ctl;
    cn.r.mask = c->cn_S ? c->buf<unsigned>(CN_MASK) : c->buf<unsigned>(CN_MASK1);
    cn.r.q = c->cn_S ? c->buf<unsigned>(CN_Q) : nullptr;
    cn.r.slot = (unsigned)slot0;
    cn.r.bias_ptr = bias_ptr ? call : nullptr; cn.r.bias_tok = call + n + 1; cn.r.bias_val = reinterpret_cast<const float *>(call + n + 1 + nb);
    cn.v.csr = csr_args(c); cn.v.q = c->buf<unsigned>(CN_Q); cn.v.slot = (unsigned)slot0; cn.v.n = (unsigned)n;
    cn.v.done = st ? call + words : nullptr; cn.v.len = st ? st->a.len : nullptr;
    cn.v.feedback = 0; cn.v.ctl = c->ctl; cn.v.gen = c->gen; cn.v.gen_cap = c->gen_cap;
    if (st) st->a.done = cn.v.done;
    if (start) {
        std::vector<unsigned> &q = cn_states(c);
        std::copy(start, start + n, q.begin() + slot0);
        HIPCHK(hipMemcpyAsync(c->buf<unsigned>(CN_Q) + slot0, q.data() + slot0, sizeof(unsigned) * n, hipMemcpyHostToDevice, c->stream));
    }
    return 0;
}
// behind the call's last launch q comes back
int constrainer_download(rwkv_ctx *c, uint64_t slot0, uint64_t n)
{
    HIPCHK(hipMemcpyAsync(cn_states(c).data() + slot0, c->buf<unsigned>(CN_Q) + slot0, sizeof(unsigned) * n, hipMemcpyDeviceToHost, c->stream));
    return 0;
}

// what a pick of kind `kind` over `rows` rows needs besides the rows: the row argmax's partials, or a scratch slice per row for a sampler
int grow_pick_buffers(rwkv_ctx *c, int kind, uint64_t rows)
{
    if (kind == RWKV_PICK_GREEDY) {
        if (const int rc = grow_buffer(c, BD_VAL, sizeof(float) * rows * AM_SLICES)) return rc;
        return grow_buffer(c, BD_IDX, sizeof(unsigned) * rows * AM_SLICES);
    }
    if (const int rc = grow_buffer(c, BD_PART, sizeof(double) * rows * TS_PART_ROW)) return rc;
    if (const int rc = grow_buffer(c, BD_P, sizeof(float) * rows * TS_ROW)) return rc;
    if (const int rc = grow_buffer(c, BD_PW, sizeof(float) * rows * TS_ROW)) return rc;
    return grow_buffer(c, BD_KEY, sizeof(unsigned) * rows * TS_ROW);
}

// ---- the run of a generation call (DecodeCall) ----
// setup; per step k: forward -> constrained rows -> pick -> automaton advance -> record -> stop test (step); end; the wait; results on the host.
// The parts a call does not ask for are absent from every one of these.  A call has one of two forms, one stream (the decode path's kernels on
// slot 0) or many (the chunk path over rows and slots 0 .. N - 1), and they differ in three things only:
//   the forward             one: the token graph, with its argmax node only where that node is the pick (greedy, no constraint);
//                           many: one rwkv_forward(N, PARRALEL) schedule whose embedding reads ids row k on the device
//   where step k's picks    one: written to c->pick and fed back through the control block -- by the graph's node, the sampler or, greedy under a
//   land                    constraint, k_constraint_advance -- which also puts them to gen[k], where the record and the stop test read them;
//                           many: ids row k + 1, which the next forward reads
//   the sampler's scratch   one: the context's single-row set, u of step k from seed + k through the control block;
//                           many: the BD_* slices, one seed per row
// One upload (one: the control block; many: [seeds | first tokens]) and one download of all picks.  A call that can stop no stream owns no Stopper
// (two small launches behind each step's pick, one behind the last) and runs all its steps; a constrained call always owns one: a stream ends
// where its automaton does.
struct DecodeRun {
    const DecodeCall &d;
    const bool one = d.N == 1, sampled = d.pick.kind != RWKV_PICK_GREEDY;
    Stopper stopper, *st = d.cp || (d.stop && (d.stop->n_seqs || d.stop->max_new)) ? &stopper : nullptr;
    LpRecorder recorder, *lp = d.lp ? &recorder : nullptr;
    Constrainer constrainer, *cn = d.cp ? &constrainer : nullptr;
    Sampler smp{};                                  // greedy: no arguments are built
    unsigned long long *ids = nullptr;              // many: ids row k, the ids fed at step k (BD_IDS behind the seeds)
    uint64_t ran() const { return st ? st->steps_run : d.n_steps; }      // steps enqueued

    // buffers, stopper, constrainer with its start states, recorder, counts, the one upload; then the sampler's arguments (no device work)
    int setup(rwkv_ctx *c, const StopTable *table)
    {
        const uint64_t N = d.N;
        if (const int rc = one ? 0 : grow_buffer(c, BD_IDS, sizeof(unsigned long long) * N * (d.n_steps + 2))) return rc;
        if (const int rc = !one || (cn && !sampled) ? grow_pick_buffers(c, d.pick.kind, N) : 0) return rc;      // (one stream: only the row argmax needs any)
        if (const int rc = st ? stopper_setup(c, *st, *table, d.stop, d.first, N, d.n_steps, true, pick_penalty(d.pick)) : 0) return rc;
        if (const int rc = cn ? constrainer_setup(c, *cn, 0, 0, N, d.cp->bias_ptr, d.cp->bias_tok, d.cp->bias_val, st, d.cp->start) : 0) return rc;
        if (const int rc = lp ? lp_setup(c, *lp, N, d.n_steps, d.lp->top_n) : 0) return rc;
        if (const int rc = pick_counts(c, d.pick, 0, N, true)) return rc;
        c->bd_host.assign(N * (d.n_steps + 1), 0ull);       // many: the upload; both: the download of the picks, [step][stream]
        if (one) {
            if (const int rc = set_ctl(c, d.first[0], 0, 0)) return rc;
        } else {
            unsigned long long *dseeds = c->buf<unsigned long long>(BD_IDS);
            ids = dseeds + N;
            for (uint64_t s = 0; s < N; s++) { c->bd_host[s] = sampled ? d.seeds[s] : 0ull; c->bd_host[N + s] = d.first[s]; }
            HIPCHK(hipMemcpyAsync(dseeds, c->bd_host.data(), sizeof(unsigned long long) * 2 * N, hipMemcpyHostToDevice, c->stream));
        }
        if (sampled) {
            smp = make_sampler(c, d.pick, true);
            if (one) smp.draw().seed = d.seeds[0];
            else sampler_to_batch(c, smp, ids - N);
            if (cn) cn->feed(smp);
        }
        if (cn) cn->v.feedback = one && !sampled ? 1 : 0;      // one stream, greedy: k_constraint_advance feeds the pick back
        return 0;
    }

    // step k; more: enqueue the next one
    int step(rwkv_ctx *c, uint64_t k, bool *more)
    {
        const unsigned n = (unsigned)d.N;
        unsigned long long *to = one ? c->pick : ids + (k + 1) * n;       // where the pick writes,
        const unsigned long long *picks = one ? c->gen + k : to;          // and where what follows it reads step k's picks
        if (const int rc = one ? run_token(c, !sampled && !cn) : enqueue_rows(c, nullptr, ids + k * n, n, RowLayout::of_mode(RWKV_MODE_PARRALEL))) return rc;      // logits rows and state slots 0 .. N - 1
        if (const int rc = cn ? cn->rows(c, n) : 0) return rc;
        if (sampled) {
            smp.draw().step = one ? -1 : (int)k; smp.draw().pick = to;
            if (const int rc = enqueue_pick(c, smp, n)) return rc;
        } else if (cn || !one) {                                          // (else the token graph's last node was the pick)
            if (const int rc = enqueue_argmax_rows(c, cn ? cn->r.out : c->logits, n, to)) return rc;
        }
        if (const int rc = cn ? cn->advance(c, to) : 0) return rc;
        if (const int rc = lp ? lp->record(c, k, picks) : 0) return rc;
        return st ? st->after_step(c, k, picks, more) : 0;
    }

    // behind the last step: record download, picks download (of the steps that ran), unpark, lengths and reasons, automaton states
    int end(rwkv_ctx *c)
    {
        if (const int rc = lp ? lp_download(c, *lp, ran()) : 0) return rc;
        HIPCHK(hipMemcpyAsync(c->bd_host.data(), one ? c->gen : ids + d.N, sizeof(unsigned long long) * d.N * ran(), hipMemcpyDeviceToHost, c->stream));
        if (const int rc = st ? st->unpark(c) : 0) return rc;
        if (const int rc = st ? stopper_download(c, *st) : 0) return rc;
        return cn ? constrainer_download(c, 0, d.N) : 0;
    }

    // behind the wait: [step][stream] -> [stream][step], lengths, reasons and the steps enqueued, 0 for the ids behind a stream's end, the record,
    // the automaton states
    void results(const rwkv_ctx *c) const
    {
        const uint64_t N = d.N, S = d.n_steps;
        for (uint64_t k = 0; k < ran(); k++)
            for (uint64_t s = 0; s < N; s++) d.out_tokens[s * S + k] = c->bd_host[k * N + s];
        stop_results(c, st != nullptr, N, S, d.out_len, d.out_reason);
        for (uint64_t s = 0; d.out_len && s < N; s++)
            for (uint64_t k = d.out_len[s]; k < S; k++) d.out_tokens[s * S + k] = 0;
        if (d.steps_run) *d.steps_run = ran();
        if (lp) lp_results(c, *d.lp, N, S, d.out_len);
        if (cn && d.cp->out_state) std::copy(c->cn_q.begin(), c->cn_q.begin() + N, d.cp->out_state);
    }
};

int run_call(rwkv_ctx *c, const DecodeCall &d, const StopTable *table)
{
    DecodeRun r{d};
    const int rc = finish(c, [&]() -> int {
        if (const int rc = r.setup(c, table)) return rc;
        bool more = true;
        for (uint64_t k = 0; k < d.n_steps && more; k++)
            if (const int rc = r.step(c, k, &more)) return rc;
        return r.end(c);
    }());
    if (!rc) r.results(c);
    return rc;
}

// the checks of rwkv_decode_batch_greedy / _typical / _nucleus / _until / _logprobs / _constrained, all of them before anything is launched
int decode_batch(rwkv_ctx *c, const DecodeCall &d)
{
    if (const int rc = guard(c, NEED_WHOLE | LAUNCHES, d.first && d.out_tokens && (d.pick.kind == RWKV_PICK_GREEDY || d.seeds))) return rc;
    if (d.N == 0 || d.N > c->maxT) return fail(RWKV_E_ARG, "n_streams must be in 1..%llu (max context)", (unsigned long long)c->maxT);
    if (const int rc = check_steps(d.n_steps, "n_steps")) return rc;
    if (const int rc = check_ids(d.first, d.N, "token")) return rc;
    if (const int rc = check_pick(d.pick)) return rc;
    StopTable table{};
    if (const int rc = d.stop ? check_stop(d.stop, d.N, d.n_steps, &table) : 0) return rc;
    if (d.lp && d.N * d.n_steps * (1 + (uint64_t)d.lp->top_n) > RWKV_MAX_LOGPROB_ENTRIES)
        return fail(RWKV_E_ARG, "n_streams * n_steps * (1 + top_n) must not exceed %u: split the generation into calls", RWKV_MAX_LOGPROB_ENTRIES);
    if (d.N >= 2 && !c->seq_ok) return fail(RWKV_E_STATE, "n_streams >= 2 needs the chunk path (off: RWKV_SEQ=0, max context 1 or n_embed not a multiple of 64)");
    if (const int rc = d.cp ? check_constrain(c, *d.cp, d.pick, d.N) : 0) return rc;
    return run_call(c, d, &table);
}

// the record's description is acceptable
int check_logprob_out(const rwkv_logprob_out &lp)
{
    if (lp.top_n > RWKV_MAX_TOPN) return fail(RWKV_E_ARG, "top_n must be in 0..%u", RWKV_MAX_TOPN);
    if ((lp.top_n > 0) != (lp.top_ids != nullptr) || (lp.top_n > 0) != (lp.top_logprob != nullptr))
        return fail(RWKV_E_ARG, "top_ids and top_logprob go with top_n > 0, and only with it");
    if (lp.reserved) return fail(RWKV_E_ARG, "reserved != 0");
    return 0;
}
} // namespace

int rwkv_decode_batch_greedy(rwkv_ctx *c, const uint64_t *first_tokens, uint64_t n_streams, uint64_t n_steps, uint64_t *out_tokens)
{
    return decode_batch(c, DecodeCall{n_streams, n_steps, first_tokens, nullptr, pick_greedy(), out_tokens});
}

int rwkv_decode_batch_typical(rwkv_ctx *c, const uint64_t *first_tokens, uint64_t n_streams, uint64_t n_steps, float temp, float tau,
                              const uint64_t *seeds, int flags, uint64_t *out_tokens)
{
    return decode_batch(c, DecodeCall{n_streams, n_steps, first_tokens, seeds, pick_typical(temp, tau, flags), out_tokens});
}

int rwkv_sample_nucleus(rwkv_ctx *c, uint64_t row, uint64_t slot, const rwkv_nucleus_params *p, double u, uint64_t *token)
{
    if (const int rc = guard(c, NEED_HEAD | LAUNCHES, p && token)) return rc;
    if (const int rc = check_row_slot(c, row, slot)) return rc;
    const rwkv_pick pk = pick_nucleus(*p);
    if (const int rc = check_pick(pk)) return rc;
    if (!(u >= 0.0 && u < 1.0)) return fail(RWKV_E_ARG, "need 0 <= u < 1");
    return finish(c, [&]() -> int {
        if (const int rc = pick_counts(c, pk, slot, 1, false)) return rc;
        Sampler s = make_sampler(c, pk, false);
        s.n.row = (int)row; s.n.slot = (unsigned)slot; s.n.u = u;
        if (const int rc = enqueue_pick(c, s, 1)) return rc;
        HIPCHK(hipMemcpyAsync(token, c->pick, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        return 0;
    }());
}

int rwkv_decode_nucleus(rwkv_ctx *c, uint64_t first_token, uint64_t n, const rwkv_nucleus_params *p, uint64_t seed, uint64_t *out_tokens)
{
    if (const int rc = guard(c, NEED_WHOLE | LAUNCHES, p && out_tokens)) return rc;
    return decode_one(c, first_token, n, pick_nucleus(*p), seed, out_tokens);
}

int rwkv_decode_batch_nucleus(rwkv_ctx *c, const uint64_t *first_tokens, uint64_t n_streams, uint64_t n_steps, const rwkv_nucleus_params *p,
                              const uint64_t *seeds, uint64_t *out_tokens)
{
    if (const int rc = guard(c, 0, p)) return rc;
    return decode_batch(c, DecodeCall{n_streams, n_steps, first_tokens, seeds, pick_nucleus(*p), out_tokens});
}

int rwkv_decode_batch_until(rwkv_ctx *c, const uint64_t *first_tokens, uint64_t n_streams, uint64_t n_steps, const rwkv_pick *pick,
                            const uint64_t *seeds, const rwkv_stop_params *stop, uint64_t *out_tokens, uint32_t *out_len, uint32_t *out_reason,
                            uint64_t *steps_run)
{
    if (const int rc = guard(c, NEED_WHOLE, pick && stop && out_len)) return rc;
    if (const int rc = check_pick_kind(*pick)) return rc;
    return decode_batch(c, DecodeCall{n_streams, n_steps, first_tokens, seeds, *pick, out_tokens, stop, out_len, out_reason, steps_run});
}

static_assert(TOPN_MAX == RWKV_MAX_TOPN, "topn.hip.h holds the header's limit");
static_assert(sizeof(rwkv_logprob_out) == 40, "rwkv_logprob_out is 40 bytes in the C ABI");
int rwkv_decode_batch_logprobs(rwkv_ctx *c, const uint64_t *first_tokens, uint64_t n_streams, uint64_t n_steps, const rwkv_pick *pick,
                               const uint64_t *seeds, const rwkv_stop_params *stop, const rwkv_logprob_out *lp, uint64_t *out_tokens,
                               uint32_t *out_len, uint32_t *out_reason, uint64_t *steps_run)
{
    if (const int rc = guard(c, NEED_WHOLE, pick && lp && lp->logprob && (!stop || out_len))) return rc;
    if (const int rc = check_logprob_out(*lp)) return rc;
    if (const int rc = check_pick_kind(*pick)) return rc;
    return decode_batch(c, DecodeCall{n_streams, n_steps, first_tokens, seeds, *pick, out_tokens, stop, out_len, out_reason, steps_run, lp});
}

int rwkv_constraint_set(rwkv_ctx *c, const rwkv_automaton *a)
{
    if (const int rc = guard(c, NEED_LOADED | LAUNCHES, a)) return rc;
    if (a->reserved) return fail(RWKV_E_ARG, "reserved != 0");
    const constraint_view view{a->n_states, a->row_ptr, a->nnz, a->tok, a->next};
    if (const char *rule = constraint_check(&view, nullptr)) return fail(RWKV_E_ARG, "malformed automaton: %s", rule);
    const size_t S = a->n_states, nnz = a->nnz;
    const int rc = finish(c, [&]() -> int {
        if (const int rc = grow_buffer(c, CN_CSR, sizeof(unsigned) * (S + 1 + 2 * nnz))) return rc;
        if (const int rc = grow_buffer(c, CN_MASK, sizeof(unsigned) * S * CN_WORDS)) return rc;
        if (const int rc = grow_buffer(c, CN_Q, sizeof(unsigned) * c->maxT)) return rc;
        unsigned *w = c->buf<unsigned>(CN_CSR);
        HIPCHK(hipMemcpyAsync(w, a->row_ptr, sizeof(unsigned) * (S + 1), hipMemcpyHostToDevice, c->stream));
        if (nnz) {
            HIPCHK(hipMemcpyAsync(w + S + 1, a->tok, sizeof(unsigned) * nnz, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(w + S + 1 + nnz, a->next, sizeof(unsigned) * nnz, hipMemcpyHostToDevice, c->stream));
        }
        k_constraint_mask<0><<<dim3((unsigned)S), dim3(CN_NT), 0, c->stream>>>(CsrArgs{w, w + S + 1, w + S + 1 + nnz, (unsigned)S}, c->buf<unsigned>(CN_MASK));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemsetAsync(c->grown[CN_Q].p, 0, sizeof(unsigned) * c->maxT, c->stream));
        return 0;
    }());
    if (rc) { c->cn_S = 0; c->cn_nnz = 0; c->cn_row_ptr.clear(); return rc; }      // (a failed upload: the buffers no longer hold the previous automaton)
    c->cn_S = (unsigned)S; c->cn_nnz = nnz;
    c->cn_row_ptr.assign(a->row_ptr, a->row_ptr + S + 1);
    c->cn_q.assign(c->maxT, 0u);
    return 0;
}

int rwkv_constraint_clear(rwkv_ctx *c)
{
    if (const int rc = guard(c, NEED_LOADED)) return rc;
    const int rc = finish(c, [&]() -> int {
        if (c->grown[CN_Q].p) HIPCHK(hipMemsetAsync(c->grown[CN_Q].p, 0, sizeof(unsigned) * c->maxT, c->stream));
        return 0;
    }());
    for (const GrownBuf b : {CN_CSR, CN_MASK}) {       // (the stream is idle)
        rwkv_ctx::Grown &g = c->grown[b];
        if (g.p) { (void)hipFree(g.p); c->alloc_bytes -= g.bytes; g.p = nullptr; g.bytes = 0; }
    }
    c->cn_S = 0; c->cn_nnz = 0; c->cn_row_ptr.clear();
    c->cn_q.assign(c->maxT, 0u);
    return rc;
}

int rwkv_constraint_state_set(rwkv_ctx *c, uint64_t slot0, uint64_t n, const uint32_t *states)
{
    if (const int rc = guard(c, NEED_LOADED, states)) return rc;
    if (const int rc = check_slot_span(c, slot0, n)) return rc;
    for (uint64_t i = 0; i < n; i++)
        if (states[i] >= std::max(c->cn_S, 1u)) return fail(RWKV_E_ARG, "automaton state %u is not below %u", states[i], std::max(c->cn_S, 1u));
    std::vector<unsigned> &q = cn_states(c);
    const int rc = finish(c, [&]() -> int {
        if (!c->grown[CN_Q].p) {
            if (const int rc = grow_buffer(c, CN_Q, sizeof(unsigned) * c->maxT)) return rc;
            HIPCHK(hipMemsetAsync(c->grown[CN_Q].p, 0, sizeof(unsigned) * c->maxT, c->stream));
        }
        HIPCHK(hipMemcpyAsync(c->buf<unsigned>(CN_Q) + slot0, states, sizeof(unsigned) * n, hipMemcpyHostToDevice, c->stream));
        return 0;
    }());
    if (!rc) std::copy(states, states + n, q.begin() + slot0);
    return rc;
}

int rwkv_constraint_state_get(rwkv_ctx *c, uint64_t slot0, uint64_t n, uint32_t *states)
{
    if (const int rc = guard(c, NEED_LOADED, states)) return rc;
    if (const int rc = check_slot_span(c, slot0, n)) return rc;
    const std::vector<unsigned> &q = cn_states(c);
    std::copy(q.begin() + slot0, q.begin() + slot0 + n, states);
    return 0;
}

int rwkv_pick_constrained(rwkv_ctx *c, uint64_t row, uint64_t slot, const rwkv_pick *pick, const rwkv_bias *bias, double u, int advance, uint64_t *token,
                          uint32_t *state_out)
{
    if (const int rc = guard(c, NEED_HEAD | LAUNCHES, pick && token)) return rc;
    if (const int rc = check_row_slot(c, row, slot)) return rc;
    if (pick->kind == RWKV_PICK_TYPICAL) return fail(RWKV_E_ARG, "typical sampling under a constraint is out of scope: pick greedy or nucleus");
    if (const int rc = check_pick(*pick)) return rc;
    const bool sampled = pick->kind == RWKV_PICK_NUCLEUS;
    if (sampled && !(u >= 0.0 && u < 1.0)) return fail(RWKV_E_ARG, "need 0 <= u < 1");
    if (bias && bias->reserved) return fail(RWKV_E_ARG, "reserved != 0");
    if (const int rc = bias ? check_bias(bias->n, bias->tok, bias->val) : 0) return rc;
    if (const int rc = check_start(c, slot, cn_states(c)[slot])) return rc;
    const uint32_t bptr[2] = {0u, bias ? bias->n : 0u};
    const int rc = finish(c, [&]() -> int {
        Constrainer cn;
        if (const int rc = constrainer_setup(c, cn, row, slot, 1, bias ? bptr : nullptr, bias ? bias->tok : nullptr, bias ? bias->val : nullptr, nullptr)) return rc;
        if (const int rc = cn.rows(c, 1)) return rc;
        if (sampled) {
            if (const int rc = pick_counts(c, *pick, slot, 1, false)) return rc;
            Sampler s = make_sampler(c, *pick, false);
            cn.feed(s);
            s.n.row = (int)row; s.n.slot = (unsigned)slot; s.n.u = u;
            if (const int rc = enqueue_pick(c, s, 1)) return rc;
        } else {
            if (const int rc = grow_pick_buffers(c, RWKV_PICK_GREEDY, 1)) return rc;
            if (const int rc = enqueue_argmax_rows(c, cn.r.out + row * RWKV_VOCAB, 1, c->pick)) return rc;
        }
        if (advance && c->cn_S) {
            if (const int rc = cn.advance(c, c->pick)) return rc;
            if (const int rc = constrainer_download(c, slot, 1)) return rc;
        }
        HIPCHK(hipMemcpyAsync(token, c->pick, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        return 0;
    }());
    if (!rc && state_out) *state_out = c->cn_q[slot];
    return rc;
}

int rwkv_debug_constrained_row(rwkv_ctx *c, uint64_t row, float *dst)
{
    if (const int rc = guard(c, NEED_LOADED, dst)) return rc;
    if (row >= c->maxT) return fail(RWKV_E_ARG, "row %llu out of range (max context %llu)", (unsigned long long)row, (unsigned long long)c->maxT);
    if (!c->grown[CN_ROWS].p) return fail(RWKV_E_STATE, "no constrained pick has run on this context");
    return finish(c, [&]() -> int {
        HIPCHK(hipMemcpyAsync(dst, c->buf<float>(CN_ROWS) + row * RWKV_VOCAB, sizeof(float) * RWKV_VOCAB, hipMemcpyDeviceToHost, c->stream));
        return 0;
    }());
}

int rwkv_decode_batch_constrained(rwkv_ctx *c, const uint64_t *first_tokens, uint64_t n_streams, uint64_t n_steps, const rwkv_pick *pick,
                                  const uint64_t *seeds, const rwkv_constrain_params *cp, const rwkv_stop_params *stop, const rwkv_logprob_out *lp,
                                  uint64_t *out_tokens, uint32_t *out_len, uint32_t *out_reason, uint64_t *steps_run)
{
    if (const int rc = guard(c, NEED_WHOLE, pick && cp && out_len && (!lp || lp->logprob))) return rc;
    if (const int rc = lp ? check_logprob_out(*lp) : 0) return rc;
    if (const int rc = check_pick_kind(*pick)) return rc;
    return decode_batch(c, DecodeCall{n_streams, n_steps, first_tokens, seeds, *pick, out_tokens, stop, out_len, out_reason, steps_run, lp, cp});
}

int rwkv_topn_rows(rwkv_ctx *c, const uint64_t *rows, uint64_t n, uint32_t top_n, uint64_t *ids, double *logprob)
{
    if (const int rc = guard(c, NEED_HEAD | LAUNCHES, rows && ids && logprob)) return rc;
    if (n == 0 || n > RWKV_MAX_SCORE) return fail(RWKV_E_ARG, "n must be in 1..%u", RWKV_MAX_SCORE);
    if (top_n == 0 || top_n > RWKV_MAX_TOPN) return fail(RWKV_E_ARG, "top_n must be in 1..%u", RWKV_MAX_TOPN);
    for (uint64_t i = 0; i < n; i++)
        if (rows[i] >= c->maxT) return fail(RWKV_E_ARG, "logits row %llu out of range (max context %llu)", (unsigned long long)rows[i], (unsigned long long)c->maxT);
    LpRecorder r;
    const int rc = finish(c, [&]() -> int {
        if (const int rc = lp_setup(c, r, n, 1, top_n)) return rc;
        unsigned long long *drows = c->buf<unsigned long long>(LP_REC);
        c->lp_host.resize(n + 2 * n * top_n);               // the upload | the download (ids | logprob: the step's pick part stays unused)
        std::copy(rows, rows + n, c->lp_host.begin());
        HIPCHK(hipMemcpyAsync(drows, c->lp_host.data(), sizeof(unsigned long long) * n, hipMemcpyHostToDevice, c->stream));
        for (uint64_t q = 0; q < n; q += SC_MAX_Y) {       // one launch sequence per SC_MAX_Y queries (gridDim.y)
            TopnArgs t = r.a;
            t.rows = drows + q; t.part += q * SC_PART_Q; t.cand += q * SC_G * top_n;
            t.ids = reinterpret_cast<unsigned long long *>(r.rec + 2 * n) + q * top_n; t.logprob = r.rec + (2 + (size_t)top_n) * n + q * top_n;
            if (const int rc = LpRecorder::launch(c, t, (unsigned)std::min<uint64_t>(n - q, SC_MAX_Y))) return rc;
        }
        HIPCHK(hipMemcpyAsync(c->lp_host.data() + n, r.rec + 2 * n, sizeof(double) * 2 * n * top_n, hipMemcpyDeviceToHost, c->stream));
        return 0;
    }());
    if (rc) return rc;
    memcpy(ids, c->lp_host.data() + n, sizeof(uint64_t) * n * top_n);
    memcpy(logprob, c->lp_host.data() + n + n * top_n, sizeof(double) * n * top_n);
    return 0;
}

int rwkv_debug_stop_scan(rwkv_ctx *c, const uint64_t *ids, const uint64_t *first_tokens, uint64_t n, uint64_t steps, const rwkv_stop_params *stop,
                         uint32_t *out_len, uint32_t *out_reason)
{
    if (const int rc = guard(c, NEED_LOADED | LAUNCHES, ids && first_tokens && stop && out_len && out_reason)) return rc;
    if (n == 0 || n > c->maxT) return fail(RWKV_E_ARG, "n must be in 1..%llu (max context)", (unsigned long long)c->maxT);
    if (const int rc = check_steps(steps, "steps")) return rc;
    if (const int rc = check_ids(first_tokens, n, "token")) return rc;
    if (const int rc = check_ids(ids, n * steps, "planted")) return rc;
    StopTable table{};
    if (const int rc = check_stop(stop, n, steps, &table)) return rc;
    Stopper st;
    const int rc = finish(c, [&]() -> int {
        if (const int rc = grow_buffer(c, BD_IDS, sizeof(unsigned long long) * n * steps)) return rc;
        if (const int rc = stopper_setup(c, st, table, stop, first_tokens, n, steps, false, false)) return rc;
        c->bd_host.resize(n * steps);
        for (uint64_t k = 0; k < steps; k++)            // [stream][step] -> [step][stream], as a generation call of many streams leaves its picks
            for (uint64_t s = 0; s < n; s++) c->bd_host[k * n + s] = ids[s * steps + k];
        unsigned long long *picks = c->buf<unsigned long long>(BD_IDS);
        HIPCHK(hipMemcpyAsync(picks, c->bd_host.data(), sizeof(unsigned long long) * n * steps, hipMemcpyHostToDevice, c->stream));
        for (uint64_t k = 0; k < steps; k++)
            k_stop_step<<<dim3((unsigned)(n + STOP_NT - 1) / STOP_NT), dim3(STOP_NT), 0, c->stream>>>(st.a, picks + k * n, (unsigned)k);
        HIPCHK(hipGetLastError());
        return stopper_download(c, st);
    }());
    if (rc) return rc;
    stop_results(c, true, n, steps, out_len, out_reason);
    return 0;
}

int rwkv_penalty_set(rwkv_ctx *c, uint64_t slot, const float *counts)
{
    if (const int rc = guard(c, NEED_LOADED)) return rc;
    if (slot >= c->maxT) return fail(RWKV_E_ARG, "slot %llu out of range (max context %llu)", (unsigned long long)slot, (unsigned long long)c->maxT);
    if (!counts && !c->grown[PEN_COUNTS].p) return 0;        // zero is what an unallocated buffer holds
    return finish(c, [&]() -> int {
        if (const int rc = counts_alloc(c)) return rc;
        float *dst = c->buf<float>(PEN_COUNTS) + slot * RWKV_VOCAB;
        if (counts) HIPCHK(hipMemcpyAsync(dst, counts, sizeof(float) * RWKV_VOCAB, hipMemcpyHostToDevice, c->stream));
        else HIPCHK(hipMemsetAsync(dst, 0, sizeof(float) * RWKV_VOCAB, c->stream));
        return 0;
    }());
}

int rwkv_penalty_get(rwkv_ctx *c, uint64_t slot, float *counts)
{
    if (const int rc = guard(c, NEED_LOADED, counts)) return rc;
    if (slot >= c->maxT) return fail(RWKV_E_ARG, "slot %llu out of range (max context %llu)", (unsigned long long)slot, (unsigned long long)c->maxT);
    if (!c->grown[PEN_COUNTS].p) { std::fill(counts, counts + RWKV_VOCAB, 0.f); return 0; }
    return finish(c, [&]() -> int {
        HIPCHK(hipMemcpyAsync(counts, c->buf<float>(PEN_COUNTS) + slot * RWKV_VOCAB, sizeof(float) * RWKV_VOCAB, hipMemcpyDeviceToHost, c->stream));
        return 0;
    }());
}

int rwkv_state_copy(rwkv_ctx *c, uint64_t dst, uint64_t src)
{
    if (const int rc = guard(c, NEED_LOADED)) return rc;
    if (dst >= c->maxT || src >= c->maxT)
        return fail(RWKV_E_ARG, "state slot out of range (dst %llu, src %llu, max context %llu)", (unsigned long long)dst, (unsigned long long)src, (unsigned long long)c->maxT);
    if (dst == src) return 0;
    const size_t n = (size_t)c->L * c->D;
    return finish(c, [&]() -> int {
        for (int s = 0; s < 5; s++)
            HIPCHK(hipMemcpyAsync(c->state[s] + dst * n, c->state[s] + src * n, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        return 0;
    }());
}

namespace {
// ---- beam search (beam.hip.h): rwkv_decode_beam, rwkv_debug_beam_step, rwkv_state_permute ----
static_assert(BEAM_MAX == RWKV_MAX_BEAM && BEAM_MAX_STOP == RWKV_BEAM_MAX_STOP, "beam.hip.h holds the header's limits");
static_assert(sizeof(rwkv_beam_params) == 24 && sizeof(rwkv_beam_out) == 32, "rwkv_beam_params is 24 bytes and rwkv_beam_out 32 in the C ABI");
// BEAM_REC in 8-byte words for width W and S steps: where the two id rows, the stop ids, cum, the ended / len words, the parent map and step 0 of
// the record start, the words of one step (parent, token u32 [2][W] | score [W] | token log-prob [W]) and of the whole buffer
struct BeamLayout {
    size_t ids, stop, cum, flags, parent, rec, step, words;
    BeamLayout(uint64_t W, uint64_t S) : ids(0), stop(2 * W), cum(stop + RWKV_BEAM_MAX_STOP), flags(cum + W), parent(flags + W), rec(parent + W), step(3 * W), words(rec + S * step) {}
};
// the width and the stop ids of a call are acceptable
int check_beam(const rwkv_ctx *c, const rwkv_beam_params *bp)
{
    if (bp->width < 2 || bp->width > RWKV_MAX_BEAM || bp->width > c->maxT)
        return fail(RWKV_E_ARG, "beam width must be in 2..%llu", (unsigned long long)std::min<uint64_t>(RWKV_MAX_BEAM, c->maxT));
    if (bp->n_stop > RWKV_BEAM_MAX_STOP) return fail(RWKV_E_ARG, "at most %u stop ids", RWKV_BEAM_MAX_STOP);
    if (bp->n_stop && !bp->stop_ids) return fail(RWKV_E_ARG, "NULL argument");
    if (bp->reserved) return fail(RWKV_E_ARG, "reserved != 0");
    if (const int rc = check_ids(bp->stop_ids, bp->n_stop, "stop")) return rc;
    for (uint32_t s = 0; s < bp->n_stop; s++)
        if (bp->stop_ids[s] == 0) return fail(RWKV_E_ARG, "stop id 0 is never generated");
    return 0;
}
// the two launches of the gather over slots 0 .. g.n - 1
int enqueue_gather(rwkv_ctx *c, const GatherArgs &g)
{
    const size_t total = 5 * g.LD / 2, per = (size_t)GATHER_NT * GATHER_PER;
    const unsigned chunks = (unsigned)std::min<size_t>(GATHER_CHUNKS_MAX, std::max<size_t>(1, (total + per - 1) / per));
    k_beam_gather<false><<<dim3(g.n, chunks), dim3(GATHER_NT), 0, c->stream>>>(g);
    k_beam_gather<true><<<dim3(g.n, chunks), dim3(GATHER_NT), 0, c->stream>>>(g);
    HIPCHK(hipGetLastError());
    return 0;
}
GatherArgs gather_args(rwkv_ctx *c, const unsigned *parent, uint64_t n)
{
    GatherArgs g{};
    for (int i = 0; i < 5; i++) g.state[i] = c->state[i];
    g.stage = c->buf<double>(BEAM_STAGE); g.parent = parent; g.n = (unsigned)n; g.LD = (size_t)c->L * c->D;
    return g;
}
// One call's search: the buffers (BEAM_REC, BEAM_STAGE, the top-n scratch of LP_REC), the host image of BEAM_REC's head and its upload -- row 0 of
// the ids = `fed`, cum, ended, len 0, the parent map `parent0` -- and the kernels' arguments
struct Beam {
    BeamLayout lay{2, 1};
    TopnArgs top{};
    BeamArgs a{};
    GatherArgs g{};
    unsigned long long *w = nullptr, *ids = nullptr;
    int setup(rwkv_ctx *c, const rwkv_beam_params &bp, uint64_t S, const uint64_t *fed, const double *cum, const uint8_t *ended, unsigned parent0)
    {
        const uint64_t W = bp.width;
        lay = BeamLayout(W, S);
        int rc = grow_buffer(c, BEAM_REC, sizeof(double) * lay.words);
        if (!rc) rc = grow_buffer(c, BEAM_STAGE, sizeof(double) * W * 5 * c->L * c->D);
        LpRecorder r;
        if (!rc) rc = lp_setup(c, r, W, 1, (uint32_t)W + 1);
        if (rc) return rc;
        top = r.a;
        top.ids = reinterpret_cast<unsigned long long *>(r.rec + 2 * W); top.logprob = r.rec + (2 + (W + 1)) * W;
        w = c->buf<unsigned long long>(BEAM_REC); ids = w + lay.ids;
        c->beam_host.assign(lay.words, 0ull);
        unsigned long long *h = c->beam_host.data();
        unsigned *flags = reinterpret_cast<unsigned *>(h + lay.flags), *parent = reinterpret_cast<unsigned *>(h + lay.parent);
        for (uint64_t m = 0; m < W; m++) {
            h[lay.ids + m] = fed[m];
            memcpy(&h[lay.cum + m], &cum[m], 8);
            flags[m] = ended && ended[m] ? 1u : 0u;
            parent[m] = parent0 == ~0u ? (unsigned)m : parent0;
        }
        for (uint32_t s = 0; s < bp.n_stop; s++) h[lay.stop + s] = bp.stop_ids[s];
        HIPCHK(hipMemcpyAsync(w, h, sizeof(double) * lay.rec, hipMemcpyHostToDevice, c->stream));
        a.W = (unsigned)W; a.n_stop = bp.n_stop; a.stop = w + lay.stop;
        a.top_ids = top.ids; a.top_lp = top.logprob;
        a.cum = reinterpret_cast<double *>(w + lay.cum);
        a.ended = reinterpret_cast<unsigned *>(w + lay.flags); a.len = a.ended + W;
        a.parent = reinterpret_cast<unsigned *>(w + lay.parent);
        g = gather_args(c, a.parent, W);
        return 0;
    }
    // behind step k's logits (rows 0 .. W - 1, fed ids row k & 1): the rows' top W + 1, the selection into step k of the record and ids row
    // (k + 1) & 1, and the gather
    int step(rwkv_ctx *c, uint64_t k)
    {
        if (const int rc = LpRecorder::launch(c, top, a.W)) return rc;
        BeamArgs s = a;
        unsigned long long *rec = w + lay.rec + k * lay.step;
        s.k = (unsigned)k; s.cur = ids + (k & 1) * a.W; s.next = ids + ((k + 1) & 1) * a.W;
        s.rec_parent = reinterpret_cast<unsigned *>(rec); s.rec_token = s.rec_parent + a.W;
        s.rec_score = reinterpret_cast<double *>(rec + a.W); s.rec_lp = s.rec_score + a.W;
        k_beam_select<BEAM_NT><<<dim3(1), dim3((a.W * (a.W + 1) + 63u) / 64u * 64u), 0, c->stream>>>(s);
        HIPCHK(hipGetLastError());
        return enqueue_gather(c, g);
    }
    // the one download: cum, ended, len, the parent map and the steps that ran, into the host image
    int download(rwkv_ctx *c, uint64_t ran)
    {
        HIPCHK(hipMemcpyAsync(c->beam_host.data() + lay.cum, w + lay.cum, sizeof(double) * (lay.rec - lay.cum + ran * lay.step), hipMemcpyDeviceToHost, c->stream));
        return 0;
    }
    // behind the wait: step k of the record in the host image
    const unsigned *h_parent(const rwkv_ctx *c, uint64_t k) const { return reinterpret_cast<const unsigned *>(c->beam_host.data() + lay.rec + k * lay.step); }
    const double *h_score(const rwkv_ctx *c, uint64_t k) const { return reinterpret_cast<const double *>(c->beam_host.data() + lay.rec + k * lay.step + a.W); }
};
} // namespace

int rwkv_decode_beam(rwkv_ctx *c, uint64_t first_token, uint64_t n_steps, const rwkv_beam_params *bp, const rwkv_beam_out *out)
{
    if (const int rc = guard(c, NEED_WHOLE | LAUNCHES, bp && out && out->tokens && out->len && out->score)) return rc;
    if (const int rc = check_beam(c, bp)) return rc;
    if (const int rc = check_steps(n_steps, "n_steps")) return rc;
    if (const int rc = check_ids(&first_token, 1, "token")) return rc;
    if (!c->seq_ok) return fail(RWKV_E_STATE, "beam search needs the chunk path (off: RWKV_SEQ=0, max context 1 or n_embed not a multiple of 64)");
    const uint64_t W = bp->width;
    Beam b;
    const int rc = finish(c, [&]() -> int {
        uint64_t fed[RWKV_MAX_BEAM];
        double cum[RWKV_MAX_BEAM];
        for (uint64_t m = 0; m < W; m++) { fed[m] = first_token; cum[m] = m ? -INFINITY : 0.0; }
        if (const int rc = b.setup(c, *bp, n_steps, fed, cum, nullptr, 0u)) return rc;
        if (const int rc = enqueue_gather(c, b.g)) return rc;                                  // the fork: slots 1 .. W - 1 <- slot 0
        for (uint64_t k = 0; k < n_steps; k++) {
            if (const int rc = enqueue_rows(c, nullptr, b.ids + (k & 1) * W, W, RowLayout::of_mode(RWKV_MODE_PARRALEL))) return rc;     // logits rows 0 .. W - 1, state slots 0 .. W - 1
            if (const int rc = b.step(c, k)) return rc;
        }
        return b.download(c, n_steps);
    }());
    if (rc) return rc;
    // backtrack: hypothesis m ends in beam m of the last step
    const unsigned long long *h = c->beam_host.data();
    const unsigned *len = reinterpret_cast<const unsigned *>(h + b.lay.flags) + W;
    for (uint64_t m = 0; m < W; m++) {
        out->len[m] = len[m];
        memcpy(&out->score[m], &h[b.lay.cum + m], 8);
        unsigned at = (unsigned)m;
        for (uint64_t k = n_steps; k-- > 0;) {
            const unsigned *par = b.h_parent(c, k);
            const bool on = k < len[m];
            out->tokens[m * n_steps + k] = on ? par[W + at] : 0ull;
            if (out->token_logprob) out->token_logprob[m * n_steps + k] = on ? b.h_score(c, k)[W + at] : 0.0;
            at = par[at] < W ? par[at] : 0u;
        }
    }
    return 0;
}

int rwkv_debug_beam_step(rwkv_ctx *c, const rwkv_beam_params *bp, const double *cum, const uint8_t *ended, const uint64_t *last,
                         uint32_t *parent, uint64_t *token, double *score, double *token_logprob, uint8_t *ended_out)
{
    if (const int rc = guard(c, NEED_WHOLE | LAUNCHES, bp && cum && ended && last && parent && token && score && token_logprob && ended_out)) return rc;
    if (const int rc = check_beam(c, bp)) return rc;
    const uint64_t W = bp->width;
    if (const int rc = check_ids(last, W, "token")) return rc;
    Beam b;
    const int rc = finish(c, [&]() -> int {
        if (const int rc = b.setup(c, *bp, 1, last, cum, ended, ~0u)) return rc;
        if (const int rc = b.step(c, 0)) return rc;
        return b.download(c, 1);
    }());
    if (rc) return rc;
    const unsigned *par = b.h_parent(c, 0), *end = reinterpret_cast<const unsigned *>(c->beam_host.data() + b.lay.flags);
    for (uint64_t m = 0; m < W; m++) {
        parent[m] = par[m]; token[m] = par[W + m];
        score[m] = b.h_score(c, 0)[m]; token_logprob[m] = b.h_score(c, 0)[W + m];
        ended_out[m] = end[m] ? 1 : 0;
    }
    return 0;
}

int rwkv_state_permute(rwkv_ctx *c, const uint32_t *parents, uint64_t n)
{
    if (const int rc = guard(c, NEED_LOADED | LAUNCHES, parents)) return rc;
    if (n == 0 || n > c->maxT) return fail(RWKV_E_ARG, "n must be in 1..%llu (max context)", (unsigned long long)c->maxT);
    for (uint64_t m = 0; m < n; m++)
        if (parents[m] >= n) return fail(RWKV_E_ARG, "parents[%llu] = %u is not below n = %llu", (unsigned long long)m, parents[m], (unsigned long long)n);
    return finish(c, [&]() -> int {
        int rc = grow_buffer(c, BEAM_REC, sizeof(double) * ((n + 1) / 2));
        if (!rc) rc = grow_buffer(c, BEAM_STAGE, sizeof(double) * n * 5 * c->L * c->D);
        if (rc) return rc;
        unsigned *map = c->buf<unsigned>(BEAM_REC);
        HIPCHK(hipMemcpyAsync(map, parents, sizeof(unsigned) * n, hipMemcpyHostToDevice, c->stream));
        return enqueue_gather(c, gather_args(c, map, n));
    }());
}

namespace {
// Scoring.  The call's device arrays: SC_IN = rows [N] | targets [N] (| control blocks), SC_OUT = logprob [N] | entropy [N] | argmax [N].
int score_grow(rwkv_ctx *c, uint64_t N, uint64_t n_ctl, uint64_t n_part)
{
    int rc = grow_buffer(c, SC_IN, sizeof(unsigned long long) * 2 * N + sizeof(Ctl) * n_ctl);
    if (!rc) rc = grow_buffer(c, SC_PART, sizeof(double) * SC_PART_Q * n_part);
    if (!rc) rc = grow_buffer(c, SC_OUT, sizeof(double) * 3 * N);
    return rc;
}
// the two score launches over queries [q0, q0 + n) of a call of N, their tuples in sc_part from its start on (one launch sequence
// per SC_MAX_Y queries: gridDim.y)
int enqueue_score(rwkv_ctx *c, uint64_t N, uint64_t q0, uint64_t n)
{
    const unsigned long long *in = c->buf<unsigned long long>(SC_IN);
    double *out = c->buf<double>(SC_OUT), *part = c->buf<double>(SC_PART);
    for (uint64_t k = 0; k < n; k += SC_MAX_Y) {
        const unsigned m = (unsigned)std::min<uint64_t>(n - k, SC_MAX_Y);
        const uint64_t q = q0 + k;
        const ScoreArgs a{c->logits, in + q, in + N + q, part + k * SC_PART_Q, out + q, out + N + q, reinterpret_cast<unsigned long long *>(out + 2 * N) + q};
        k_score_part<<<dim3(SC_G, m), dim3(SC_NT), 0, c->stream>>>(a);
        k_score_finish<<<dim3(m), dim3(64), 0, c->stream>>>(a);
    }
    HIPCHK(hipGetLastError());
    return 0;
}
// The exit of a scoring call: the one download of its results (into the last 3 N words of sc_host, behind what was uploaded from it) where
// `rc` says that everything before it was enqueued, the wait, and the results into the caller's arrays
int score_finish(rwkv_ctx *c, uint64_t N, int rc, double *logprob, double *entropy, uint64_t *argmax)
{
    unsigned long long *h = rc ? nullptr : c->sc_host.data() + (c->sc_host.size() - 3 * N);
    if (!rc && hipMemcpyAsync(h, c->buf<void>(SC_OUT), sizeof(double) * 3 * N, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        rc = fail(RWKV_E_DEVICE, "download of the scores failed");
    if ((rc = finish(c, rc))) return rc;
    memcpy(logprob, h, sizeof(double) * N);
    if (entropy) memcpy(entropy, h + N, sizeof(double) * N);
    if (argmax) for (uint64_t i = 0; i < N; i++) argmax[i] = h[2 * N + i];
    return 0;
}
} // namespace

int rwkv_score_rows(rwkv_ctx *c, const uint64_t *rows, const uint64_t *targets, uint64_t n, double *logprob, double *entropy, uint64_t *argmax)
{
    if (const int rc = guard(c, NEED_HEAD | LAUNCHES, rows && targets && logprob)) return rc;
    if (n == 0 || n > RWKV_MAX_SCORE) return fail(RWKV_E_ARG, "n must be in 1..%u", RWKV_MAX_SCORE);
    for (uint64_t i = 0; i < n; i++)
        if (rows[i] >= c->maxT) return fail(RWKV_E_ARG, "logits row %llu out of range (max context %llu)", (unsigned long long)rows[i], (unsigned long long)c->maxT);
    if (const int rc = check_ids(targets, n, "target")) return rc;
    return score_finish(c, n, [&]() -> int {
        if (const int rc = score_grow(c, n, 0, n)) return rc;
        c->sc_host.resize(5 * n);                       // the upload | the download
        for (uint64_t i = 0; i < n; i++) { c->sc_host[i] = rows[i]; c->sc_host[n + i] = targets[i]; }
        HIPCHK(hipMemcpyAsync(c->buf<void>(SC_IN), c->sc_host.data(), sizeof(unsigned long long) * 2 * n, hipMemcpyHostToDevice, c->stream));
        return enqueue_score(c, n, 0, n);
    }(), logprob, entropy, argmax);
}

int rwkv_score(rwkv_ctx *c, const uint64_t *tokens, const uint64_t *targets, uint64_t n, double *logprob, double *entropy, uint64_t *argmax)
{
    if (const int rc = guard(c, NEED_WHOLE | LAUNCHES, tokens && targets && logprob)) return rc;
    if (n == 0 || n > RWKV_MAX_SCORE) return fail(RWKV_E_ARG, "n_tokens must be in 1..%u", RWKV_MAX_SCORE);
    if (const int rc = check_ids(tokens, n, "token")) return rc;
    if (const int rc = check_ids(targets, n, "target")) return rc;
    trim_pass_graphs(c);
    // the pieces a caller's loop of rwkv_forward(max_ctx tokens, GPT) would make, each through the path rwkv_forward takes for it: the chunk
    // path for >= 2 tokens where the context has one, else token by token through the decode kernels
    const uint64_t P = c->maxT;
    auto chunked = [&](uint64_t np) { return np >= 2 && c->seq_ok; };
    uint64_t n_ctl = 0;
    for (uint64_t t0 = 0; t0 < n; t0 += P) { const uint64_t np = std::min(P, n - t0); if (!chunked(np)) n_ctl += np; }
    return score_finish(c, n, [&]() -> int {
        if (const int rc = score_grow(c, n, n_ctl, std::min(P, n))) return rc;
        // one upload: the logits row of every query (its position in its piece), the targets, and the control block of every token that runs
        // token by token (rwkv_forward stages those one by one in pinned memory; here they reach c->ctl by device-to-device copies)
        static_assert(sizeof(Ctl) % sizeof(unsigned long long) == 0, "control blocks sit behind the u64 arrays");
        constexpr size_t CW = sizeof(Ctl) / sizeof(unsigned long long);
        const size_t up = 2 * n + CW * n_ctl;
        c->sc_host.assign(up + 3 * n, 0ull);             // the upload | the download
        Ctl *h_ctl = reinterpret_cast<Ctl *>(c->sc_host.data() + 2 * n);
        const Ctl *d_ctl = reinterpret_cast<const Ctl *>(c->buf<unsigned long long>(SC_IN) + 2 * n);
        for (uint64_t t0 = 0, k = 0; t0 < n; t0 += P) {
            const uint64_t np = std::min(P, n - t0);
            for (uint64_t t = 0; t < np; t++) {
                c->sc_host[t0 + t] = t; c->sc_host[n + t0 + t] = targets[t0 + t];
                if (!chunked(np)) { Ctl &h = h_ctl[k++]; h.token = tokens[t0 + t]; h.slot = 0u; h.out_row = (unsigned)t; h.step = 0; h.pad = 0; }
            }
        }
        HIPCHK(hipMemcpyAsync(c->buf<void>(SC_IN), c->sc_host.data(), sizeof(unsigned long long) * up, hipMemcpyHostToDevice, c->stream));
        for (uint64_t t0 = 0, k = 0; t0 < n; t0 += P) {
            const uint64_t np = std::min(P, n - t0);
            if (chunked(np)) { if (const int rc = enqueue_rows(c, tokens + t0, nullptr, np, RowLayout::of_mode(RWKV_MODE_GPT))) return rc; }
            else
                for (uint64_t t = 0; t < np; t++) {
                    HIPCHK(hipMemcpyAsync(c->ctl, d_ctl + k++, sizeof(Ctl), hipMemcpyDeviceToDevice, c->stream));
                    if (const int rc = run_token(c, false)) return rc;
                }
            if (const int rc = enqueue_score(c, n, t0, np)) return rc;      // behind the piece, in front of the next one, which overwrites the rows
        }
        return 0;
    }(), logprob, entropy, argmax);
}

namespace {
// ---- speculative greedy decoding (spec.hip.h): rwkv_spec_verify, rwkv_decode_speculative ----
static_assert(SPEC_MAX_DRAFT == RWKV_SPEC_MAX_DRAFT, "spec.hip.h holds the header's limit");
SeqCkptFns seq_ckpt_fns() { return SeqCkptFns{k_seq_site<3, true>, k_seq_site<2, true>, k_seq_wkv<SEQ_T, true>}; }

// the buffers a verify of n rows needs: checkpoints, record and picks, the row argmax's partials
int spec_buffers(rwkv_ctx *c, uint64_t n)
{
    if (const int rc = grow_buffer(c, SPEC_CKPT, sizeof(double) * 4 * c->L * n * c->D)) return rc;
    if (const int rc = grow_buffer(c, SPEC_REC, sizeof(unsigned long long) * (2 + SEQ_T))) return rc;
    return grow_pick_buffers(c, RWKV_PICK_GREEDY, n);
}

// Everything of one verify but the wait: ids up, the checkpointing pass over rows [token, draft ..] on slot 0, the pick of every row, what stands,
// the commit of that row, and the record's download into rec[2].  No host synchronisation in between: k_spec_commit reads a where k_spec_accept
// left it.  The pass is LAUNCHED DIRECTLY, not replayed as a captured graph under a key of its own.  Measured at 7B both ways
// (profiles/spec/graph_vs_direct.txt), the replay was never the faster one: 0.01 - 0.02 ms slower up to 16 rows, which is what the runs differ by
// among themselves, and 0.06 ms slower at 32 rows, which is not.  With nothing to gain the simpler form is kept: one pass per call, with the
// call's wait behind it, leaves the host nothing to fall behind with.
int enqueue_verify(rwkv_ctx *c, uint64_t token, const uint64_t *draft, uint64_t n_draft, unsigned long long *rec)
{
    const int n = (int)n_draft + 1;
    if (const int rc = spec_buffers(c, (uint64_t)n)) return rc;
    uint64_t rows[SEQ_T];
    rows[0] = token;
    for (uint64_t i = 0; i < n_draft; i++) rows[i + 1] = draft[i];
    if (const int rc = upload_chunk_tokens(c, rows, n, 0, c->stream)) return rc;
    double *ck = c->buf<double>(SPEC_CKPT);
    unsigned long long *drec = c->buf<unsigned long long>(SPEC_REC), *picks = drec + 2;
    const SeqPass pass{c->l0, c->l1, c->stream, &c->sp_scratch[0], 0, n, 0, token_slot(c, 0), RowLayout::checkpoints(ck)};
    if (const int rc = enqueue_chunk(c, pass)) return rc;
    if (const int rc = enqueue_argmax_rows(c, c->logits, (unsigned)n, picks)) return rc;
    k_spec_accept<64><<<dim3(1), dim3(64), 0, c->stream>>>(SpecAcceptArgs{token_slot(c, 0), picks, drec, (unsigned)n_draft});
    const SpecCommitArgs ca{drec, ck, c->state[0], c->state[1], c->state[2], c->state[4], (unsigned)c->L, (unsigned)c->D, (unsigned)n};
    k_spec_commit<SPEC_COMMIT_NT><<<dim3((unsigned)((c->L * c->D + SPEC_COMMIT_NT - 1) / SPEC_COMMIT_NT)), dim3(SPEC_COMMIT_NT), 0, c->stream>>>(ca);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rec, drec, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    return 0;
}
// the checks of a verify behind the guard, all of them before anything is launched
int check_verify(const rwkv_ctx *c, uint64_t token, const uint64_t *draft, uint64_t n_draft)
{
    if (n_draft > RWKV_SPEC_MAX_DRAFT || n_draft + 1 > c->maxT)
        return fail(RWKV_E_ARG, "n_draft must be in 0..%llu (one half of a pass, and max context - 1)", (unsigned long long)std::min<uint64_t>(RWKV_SPEC_MAX_DRAFT, c->maxT - 1));
    if (n_draft && !draft) return fail(RWKV_E_ARG, "NULL argument");
    if (const int rc = check_ids(&token, 1, "token")) return rc;
    return check_ids(draft, n_draft, "draft");
}
} // namespace

int rwkv_spec_verify(rwkv_ctx *c, uint64_t token, const uint64_t *draft, uint64_t n_draft, uint64_t *n_accepted, uint64_t *next_token)
{
    if (const int rc = guard(c, NEED_WHOLE | NEED_SEQ | LAUNCHES, n_accepted && next_token)) return rc;
    if (const int rc = check_verify(c, token, draft, n_draft)) return rc;
    unsigned long long rec[2] = {0ull, 0ull};
    const int rc = finish(c, enqueue_verify(c, token, draft, n_draft, rec));
    if (!rc) { *n_accepted = rec[0]; *next_token = rec[1]; }
    return rc;
}

int rwkv_decode_speculative(rwkv_ctx *c, rwkv_ctx *dc, uint64_t first_token, uint64_t n_tokens, uint32_t k, uint64_t *out_tokens, rwkv_spec_stats *stats)
{
    if (const int rc = guard(c, NEED_WHOLE | NEED_SEQ | LAUNCHES, dc && out_tokens)) return rc;
    if (dc == c) return fail(RWKV_E_ARG, "the draft context must be another context than the target");
    if (const int rc = guard(dc, NEED_WHOLE | LAUNCHES)) return rc;
    if (dc->device != c->device) return fail(RWKV_E_ARG, "the draft context is on device %d, the target on device %d", dc->device, c->device);
    if (k == 0 || k > RWKV_SPEC_MAX_DRAFT) return fail(RWKV_E_ARG, "k must be in 1..%u", RWKV_SPEC_MAX_DRAFT);
    if (dc->maxT < (uint64_t)k + 2) return fail(RWKV_E_ARG, "the draft context needs max context >= k + 2 = %u (a state slot per draft step)", k + 2);
    if ((uint64_t)k + 1 > c->maxT) return fail(RWKV_E_ARG, "the target context needs max context >= k + 1 = %u", k + 1);
    if (const int rc = check_steps(n_tokens, "n_tokens")) return rc;
    if (const int rc = check_ids(&first_token, 1, "token")) return rc;
    const size_t LD = (size_t)dc->L * dc->D;
    // the draft's slot `dst` <- its slot `src`, on its stream
    auto draft_copy = [&](uint64_t dst, uint64_t src) -> int {
        for (int s = 0; s < 5; s++)
            HIPCHK(hipMemcpyAsync(dc->state[s] + dst * LD, dc->state[s] + src * LD, LD * sizeof(double), hipMemcpyDeviceToDevice, dc->stream));
        return 0;
    };
    rwkv_spec_stats sts{0, 0, 0};
    uint64_t done = 0, token = first_token, last_row = 0;
    unsigned long long draft[SEQ_T], rec[2];
    // One round: the draft model's kd + 1 greedy steps on its slot 0 with a copy of slot 0 into slot i + 1 behind step i (the last step only
    // consumes draft[kd - 1]: slot kd + 1 is what the draft holds when all of it stands), the drafts' download; the verify with its 16-byte
    // download; the draft's slot 0 back from slot a + 1.  Two waits, and the restore runs under the next round's first step.
    int rc = 0;
    while (!rc && done < n_tokens) {
        const uint64_t kd = std::min<uint64_t>(k, n_tokens - done - 1);
        rc = set_ctl(dc, token, 0, 0);
        for (uint64_t i = 0; !rc && i <= kd; i++) {
            rc = run_token(dc, true);
            if (!rc) rc = draft_copy(i + 1, 0);
        }
        if (!rc && kd) rc = [&]() -> int { HIPCHK(hipMemcpyAsync(draft, dc->gen, kd * sizeof(unsigned long long), hipMemcpyDeviceToHost, dc->stream)); return 0; }();
        if (kd || rc) rc = finish(dc, rc);
        if (rc) break;
        rc = finish(c, enqueue_verify(c, token, reinterpret_cast<const uint64_t *>(draft), kd, rec));
        if (rc) break;
        const uint64_t a = rec[0];
        rc = draft_copy(0, a + 1);
        for (uint64_t i = 0; i < a; i++) out_tokens[done + i] = draft[i];
        out_tokens[done + a] = rec[1];
        done += a + 1; token = rec[1]; last_row = a;
        sts.rounds++; sts.drafted += kd; sts.accepted += a;
    }
    // the row the last id was picked from -> row 0, where a one-stream call leaves it
    if (!rc && last_row) rc = [&]() -> int { HIPCHK(hipMemcpyAsync(c->logits, c->logits + last_row * RWKV_VOCAB, RWKV_VOCAB * sizeof(float), hipMemcpyDeviceToDevice, c->stream)); return 0; }();
    rc = finish(dc, rc);
    rc = finish(c, rc);
    if (!rc && stats) *stats = sts;
    return rc;
}

// ---- segmented forward (segments.hip.h): rwkv_segment_plan, rwkv_forward_segments ----
static_assert(sizeof(rwkv_segment) == 8 && sizeof(SegRow) == 8, "rwkv_segment and a row of the plan are two 32-bit words");
namespace {
SegFns seg_fns() { return SegFns{k_seg_site<3>, k_seg_site<2>, k_seg_wkv<SEQ_T>, k_seg_wkv<SEQ_TM>, k_seg_stage<1>}; }

// The one validator and planner: the rules of a segment list, then -- into whichever outputs are there -- the plan for passes of `pass_rows` rows.
// A piece ends where its segment ends or where the pass ends.  Nothing is written when the list is rejected.
int segment_plan(const rwkv_segment *segs, uint64_t n_segs, uint64_t max_ctx, uint64_t pass_rows, uint32_t *row_slot, uint8_t *row_flags, SegRow *rows,
                 uint64_t *last_row, uint64_t *n_rows)
{
    if (!segs) return fail(RWKV_E_ARG, "NULL argument");
    if (n_segs == 0 || n_segs > max_ctx) return fail(RWKV_E_ARG, "n_segs must be in 1..%llu (max context)", (unsigned long long)max_ctx);
    uint64_t T = 0;
    for (uint64_t i = 0; i < n_segs; i++) {
        if (segs[i].n == 0) return fail(RWKV_E_ARG, "segment %llu is empty", (unsigned long long)i);
        if (segs[i].slot >= max_ctx) return fail(RWKV_E_ARG, "segment %llu: slot %u out of range, max context is %llu", (unsigned long long)i, segs[i].slot, (unsigned long long)max_ctx);
        T += segs[i].n;
        if (T > max_ctx) return fail(RWKV_E_ARG, "Context too large, max context is %llu", (unsigned long long)max_ctx);
    }
    std::vector<uint32_t> slots(n_segs);
    for (uint64_t i = 0; i < n_segs; i++) slots[i] = segs[i].slot;
    std::sort(slots.begin(), slots.end());
    for (uint64_t i = 1; i < n_segs; i++)
        if (slots[i] == slots[i - 1]) return fail(RWKV_E_ARG, "slot %u is named twice: the slots of one call are pairwise distinct", slots[i]);
    uint64_t j = 0;
    for (uint64_t i = 0; i < n_segs; i++) {
        for (uint32_t k = 0; k < segs[i].n; k++, j++) {
            const unsigned f = ((k == 0 || j % pass_rows == 0) ? SEG_FIRST : 0u) | ((k + 1 == segs[i].n || (j + 1) % pass_rows == 0) ? SEG_LAST : 0u);
            if (row_slot) row_slot[j] = segs[i].slot;
            if (row_flags) row_flags[j] = (uint8_t)f;
            if (rows) rows[j] = SegRow{segs[i].slot, f};
        }
        if (last_row) last_row[i] = j - 1;
    }
    if (n_rows) *n_rows = T;
    return 0;
}
} // namespace

int rwkv_segment_plan(const rwkv_segment *segs, uint64_t n_segs, uint64_t max_ctx, uint32_t *row_slot, uint8_t *row_flags, uint64_t *n_rows)
{
    return segment_plan(segs, n_segs, max_ctx, (uint64_t)SEQ_TM, row_slot, row_flags, nullptr, nullptr, n_rows);
}

int rwkv_forward_segments(rwkv_ctx *c, const uint64_t *tokens, const rwkv_segment *segs, uint64_t n_segs, uint32_t flags, uint64_t *last_row)
{
    if (const int rc = guard(c, NEED_WHOLE | NEED_SEQ | LAUNCHES, tokens && segs)) return rc;
    if (flags) return fail(RWKV_E_ARG, "flags must be 0");
    uint64_t T = 0;
    if (const int rc = segment_plan(segs, n_segs, c->maxT, 1, nullptr, nullptr, nullptr, nullptr, &T)) return rc;      // the rules alone
    if (const int rc = check_ids(tokens, T, "token")) return rc;
    if (!c->h_seg_plan) HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&c->h_seg_plan), sizeof(SegRow) * c->maxT, hipHostMallocDefault));
    if (const int rc = grow_buffer(c, SEG_PLAN, sizeof(SegRow) * c->maxT)) return rc;
    // (the pinned plan is free: every call that read it has returned behind its wait)
    (void)segment_plan(segs, n_segs, c->maxT, seq_pass_rows(c, T), nullptr, nullptr, c->h_seg_plan, last_row, nullptr);
    return finish(c, [&]() -> int {
        SegRow *plan = c->buf<SegRow>(SEG_PLAN);
        HIPCHK(hipMemcpyAsync(plan, c->h_seg_plan, sizeof(SegRow) * T, hipMemcpyHostToDevice, c->stream));
        return enqueue_rows(c, tokens, nullptr, T, RowLayout::segments(plan));
    }());
}

void rwkv_free(rwkv_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->g_fwd) { (void)hipGraphExecDestroy(c->g_fwd); c->g_fwd = nullptr; }
    if (c->g_greedy) { (void)hipGraphExecDestroy(c->g_greedy); c->g_greedy = nullptr; }
    rwkv_pipe_free(c);        // (no graphs left to re-capture)
    for (void *p : c->allocs) (void)hipFree(p);
    for (const rwkv_ctx::Grown &g : c->grown) if (g.p) (void)hipFree(g.p);
    if (c->h_ctl) (void)hipHostFree(c->h_ctl);
    if (c->h_seg_plan) (void)hipHostFree(c->h_seg_plan);
    if (c->herr) (void)hipHostFree(c->herr);
    for (auto &e : c->xs_ev) if (e) (void)hipEventDestroy(e);
    for (auto &e : c->hop_ev) if (e) (void)hipEventDestroy(e);
    for (auto &row : c->sp_done) for (auto &e : row) if (e) (void)hipEventDestroy(e);
    if (c->sp_end) (void)hipEventDestroy(c->sp_end);
    for (int k = 1; k < rwkv_ctx::SPLIT_MAX; k++) { if (c->sp_stream[k]) (void)hipStreamDestroy(c->sp_stream[k]); }
    for (auto &kv : c->sq_graphs) (void)hipGraphExecDestroy(kv.second);
    c->sq_graphs.clear();
    if (c->h_sq_tokens) (void)hipHostFree(c->h_sq_tokens);
    if (c->stop_ring) (void)hipHostFree(c->stop_ring);
    for (auto &e : c->stop_ev) if (e) (void)hipEventDestroy(e);
    for (int r = 0; r < SQ_RING; r++) if (c->sq_ev[r]) (void)hipEventDestroy(c->sq_ev[r]);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

float *rwkv_logits_device(rwkv_ctx *c) { return c ? c->logits : nullptr; }
double *rwkv_state_device(rwkv_ctx *c, int which) { return (c && which >= 0 && which < 5) ? c->state[which] : nullptr; }
void *rwkv_stream(rwkv_ctx *c) { return c ? (void *)c->stream : nullptr; }
int rwkv_abi_version(void) { return RWKV_MI355X_ABI_VERSION; }
uint64_t rwkv_resident_bytes(const rwkv_ctx *c) { return c ? (uint64_t)c->alloc_bytes : 0; }
int rwkv_decode_form(const rwkv_ctx *c) { return c && c->loaded ? (c->tile > 0 ? c->tile : 0) : -1; }

uint64_t rwkv_bytes_per_token(const rwkv_ctx *c)
{
    if (!c) return 0;
    const uint64_t nl = (c->l1 == UINT64_MAX ? c->L : c->l1) - c->l0, D = c->D, V = RWKV_VOCAB;
    return 13 * nl * D * D + (c->l1 == c->L || c->l1 == UINT64_MAX ? V * D : 0) + 168 * nl * D + 40 * D;   // SURVEY.md section 8(d), this stage's share
}

namespace {
// the events of a profiling call: destroyed however the call ends (as load_common's Scratch frees its staging)
struct Events {
    std::vector<hipEvent_t> ev;
    int create(size_t n)
    {
        for (ev.reserve(n); ev.size() < n;) { hipEvent_t e; HIPCHK(hipEventCreate(&e)); ev.push_back(e); }
        return 0;
    }
    ~Events() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
};
} // namespace

int rwkv_profile_token(rwkv_ctx *c, uint64_t token, int reps, double *ms, uint64_t *bytes, uint32_t *launches)
{
    if (const int rc = guard(c, NEED_LOADED | LAUNCHES, ms)) return rc;
    if (token >= RWKV_VOCAB || reps <= 0) return fail(RWKV_E_ARG, "bad token / reps");
    const uint64_t D = c->D;
    const int nlay = (int)(c->l1 - c->l0), nev = 4 * nlay + 4;
    Events evs;
    for (int k = 0; k < RWKV_N_KCLASS; k++) ms[k] = 0.0;
    const int rc = finish(c, [&]() -> int {
        if (const int rc = evs.create(nev)) return rc;
        if (const int rc = set_ctl(c, token, 0, 0)) return rc;
        for (int rep = 0; rep < reps; rep++) {
            if (const int rc = enqueue_token(c, true, evs.ev.data())) return rc;
            HIPCHK(hipStreamSynchronize(c->stream));
            for (int i = 0; i + 1 < nev; i++) {
                float t = 0.f;
                HIPCHK(hipEventElapsedTime(&t, evs.ev[i], evs.ev[i + 1]));
                int cls;
                if (i == 0) cls = 0;
                else if (i <= 4 * nlay) cls = 1 + (i - 1) % 4;
                else if (i == 4 * nlay + 1) cls = 5;
                else cls = 6;
                ms[cls] += (double)t;
            }
        }
        return 0;
    }());
    if (bytes) {
        bytes[0] = 4 * D; bytes[6] = 0;
        for (int k = 0; k < 5; k++) bytes[1 + k] = c->wc[k].row_bytes(D);
    }
    if (launches) {
        launches[0] = 1; launches[1] = launches[2] = launches[3] = launches[4] = (uint32_t)(c->l1 - c->l0); launches[5] = 1; launches[6] = 1;
    }
    return rc;
}

// Per-class launch duration from ONE event pair around a batch of back-to-back launches of that
// class (all L layers x reps): amortises the ~2.5 us a hipEvent pair adds per bracket, so the
// figure is comparable with rocprofv3's kernel durations.  ms[c] = total ms, n[c] = launches.
int rwkv_profile_batched(rwkv_ctx *c, uint64_t token, int reps, double *ms, uint32_t *n)
{
    if (const int rc = guard(c, NEED_LOADED | LAUNCHES, ms && n)) return rc;
    if (token >= RWKV_VOCAB || reps <= 0) return fail(RWKV_E_ARG, "bad token / reps");
    Events evs;
    return finish(c, [&]() -> int {
        if (const int rc = set_ctl(c, token, 0, 0)) return rc;
        if (const int rc = enqueue_token(c, true, nullptr)) return rc;   // valid inputs for every class
        if (const int rc = evs.create(2)) return rc;
        const hipEvent_t a = evs.ev[0], b = evs.ev[1];
        for (int cls = 0; cls < RWKV_N_KCLASS; cls++) {
            const bool per_layer = cls >= 1 && cls <= 4;
            // a class with ONE launch per token gets 8 x as many repetitions (4 launches in a bracket measured +10 % on k_head) and a
            // warm-up launch.  k_head's 206 MB would stay in the 256 MiB Infinity Cache between back-to-back launches (33.6 us against
            // 35.7 us inside the real token, rocprofv3): every head launch is preceded by ffn_v launches of four rotating layers (what a
            // token puts in front of it) and the same sequence WITHOUT the head is timed as well; the difference is the head.
            const int nrep = per_layer ? reps : reps * 8;
            const uint64_t nl = c->l1 - c->l0;
            const bool flush = cls == 5 && nl >= 4;
            float t = 0.f, t0 = 0.f;
            uint32_t cnt = 0;
            for (int pass = flush ? 0 : 1; pass < 2; pass++) {      // pass 0: the flushing launches alone
                launch_class(c, cls, per_layer ? c->l0 : 0);
                HIPCHK(hipStreamSynchronize(c->stream));
                HIPCHK(hipEventRecord(a, c->stream));
                cnt = 0;
                for (int r = 0; r < nrep; r++)
                    for (uint64_t l = (per_layer ? c->l0 : 0); l < (per_layer ? c->l1 : 1); l++) {
                        if (flush) for (int q = 0; q < 4; q++) launch_class(c, 4, c->l0 + (uint64_t)(4 * r + q) % nl);
                        if (pass == 1) launch_class(c, cls, l);
                        cnt++;
                    }
                HIPCHK(hipEventRecord(b, c->stream));
                HIPCHK(hipEventSynchronize(b));
                HIPCHK(hipEventElapsedTime(pass == 0 ? &t0 : &t, a, b));
            }
            ms[cls] = (double)(t - t0); n[cls] = cnt;
        }
        HIPCHK(hipGetLastError());
        // the batches above advanced the recurrent state with a scrambled schedule: reset it
        return enqueue_reset(c);
    }());
}

// debug: run one eager token with the phase timeline of the middle layer's ffn_rk kernel enabled;
// out receives grid*NW*8 100-MHz wall-clock stamps (see tl_stamp in kernels.hip.h)
int rwkv_debug_timeline(rwkv_ctx *c, uint64_t token, unsigned long long *out, uint64_t cap)
{
    if (const int rc = guard(c, NEED_LOADED | LAUNCHES, out)) return rc;
    const size_t n = (size_t)(c->grid > 512 ? c->grid : 512) * NW * 8;      // (a chunk GEMM may launch more workgroups than the decode grid)
    if (cap < n) return fail(RWKV_E_ARG, "need room for %zu stamps", n);
    return finish(c, [&]() -> int {
        if (!c->tl) { int rc = dalloc(c, &c->tl, n); if (rc) return rc; }
        HIPCHK(hipMemsetAsync(c->tl, 0, n * 8, c->stream));
        if (const int rc = set_ctl(c, token, 0, 0)) return rc;
        { const char *e = getenv("RWKV_TL_CLASS"); c->tl_cls = e ? atoi(e) : 3; }
        c->tl_on = true;
        int rc;
        if (c->tl_cls >= 10) {          // a GEMM of the chunk path (10 + kind: one 32-row GPT chunk of this token; 20 + kind: a 64-row pass, the two-half GEMMs)
            if (!c->seq_ok) { c->tl_on = false; return fail(RWKV_E_STATE, "the chunk path is not loaded (max_ctx 1)"); }
            uint64_t toks[SEQ_TM];
            for (int t = 0; t < SEQ_TM; t++) toks[t] = token;
            int rows = SEQ_T;
            if (c->tl_cls >= 20) { c->tl_cls -= 10; if (c->seq_rows > SEQ_T && c->maxT >= (uint64_t)SEQ_TM) rows = SEQ_TM; }
            rc = enqueue_whole(c, toks, rows, 0, 0);
        } else rc = enqueue_token(c, false, nullptr);
        c->tl_on = false;
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(out, c->tl, n * 8, hipMemcpyDeviceToHost, c->stream));
        return 0;
    }());
}

// ---- per-kernel parity hooks (tests/test_kernels_gpu.py): the PRODUCTION launch of one decode kernel class, eagerly, on whatever the
// context's buffers hold, and access to the intermediate vectors the kernels hand to each other.  A token is rwkv_debug_launch(0),
// then (1, 2, 3, 4) per layer, then 5: exactly what enqueue_token launches, one kernel at a time. ----
int rwkv_debug_launch(rwkv_ctx *c, int cls, uint64_t layer, uint64_t token, uint32_t slot)
{
    if (const int rc = guard(c, NEED_LOADED | LAUNCHES)) return rc;
    if (cls < 0 || cls > 6) return fail(RWKV_E_ARG, "kernel class %d out of range (0 first, 1 att, 2 att_out, 3 ffn r+k, 4 ffn_v, 5 head, 6 argmax)", cls);
    if (cls >= 1 && cls <= 4 && (layer < c->l0 || layer >= c->l1)) return fail(RWKV_E_ARG, "layer %llu is not one of this context's", (unsigned long long)layer);
    if (cls >= 5 && c->l1 != c->L) return fail(RWKV_E_STATE, "this context does not hold the head");
    if (slot >= c->maxT) return fail(RWKV_E_ARG, "state slot %u out of range", slot);
    if (const int rc = check_ids(&token, c->l0 == 0, "token")) return rc;
    return finish(c, [&]() -> int {
        if (cls == 0) {      // the token's control block: every later launch of the token reads slot / out_row from it
            if (const int rc = set_ctl(c, token, slot, slot)) return rc;
        }
        launch_class(c, cls, layer);
        HIPCHK(hipGetLastError());
        return 0;
    }());
}

namespace {
// device address and byte size of intermediate buffer `which` (enum rwkv_debug_buf)
int debug_buf(rwkv_ctx *c, int which, void **p, size_t *bytes)
{
    const size_t D = (size_t)c->D, G = (size_t)c->grid;
    switch (which) {
    case RWKV_DBG_X: *p = c->x; *bytes = D * 8; break;
    case RWKV_DBG_YBUF: *p = c->ybuf; *bytes = D * 4; break;
    case RWKV_DBG_PART_ATT: *p = c->partA; *bytes = G * 8; break;
    case RWKV_DBG_PMAX_ATT: *p = c->partMA; *bytes = G * 4; break;
    case RWKV_DBG_HBUF: *p = c->hbuf; *bytes = 4 * D * 4; break;
    case RWKV_DBG_RGATE: *p = c->rgate; *bytes = D * 4; break;
    case RWKV_DBG_PART_FFN: *p = c->partF; *bytes = G * 8; break;
    case RWKV_DBG_PMAX_FFN: *p = c->partMF; *bytes = G * 4; break;
    case RWKV_DBG_LNSTAT: *p = c->lnstat; *bytes = 6 * 8; break;
    default: return fail(RWKV_E_ARG, "no such debug buffer: %d", which);
    }
    return 0;
}
} // namespace

int rwkv_debug_read(rwkv_ctx *c, int which, void *dst, uint64_t cap)
{
    if (const int rc = guard(c, NEED_LOADED, dst)) return rc;
    void *p = nullptr; size_t n = 0;
    if (const int rc = debug_buf(c, which, &p, &n)) return rc;
    if (cap < n) return fail(RWKV_E_ARG, "debug buffer %d holds %zu bytes", which, n);
    return finish(c, [&]() -> int {
        HIPCHK(hipMemcpyAsync(dst, p, n, hipMemcpyDeviceToHost, c->stream));
        return 0;
    }());
}

int rwkv_debug_write(rwkv_ctx *c, int which, const void *src, uint64_t bytes)
{
    if (const int rc = guard(c, NEED_LOADED, src)) return rc;
    void *p = nullptr; size_t n = 0;
    if (const int rc = debug_buf(c, which, &p, &n)) return rc;
    if (bytes != n) return fail(RWKV_E_ARG, "debug buffer %d holds %zu bytes", which, n);
    return finish(c, [&]() -> int {
        HIPCHK(hipMemcpyAsync(p, src, n, hipMemcpyHostToDevice, c->stream));
        return 0;
    }());
}

uint64_t rwkv_debug_grid(const rwkv_ctx *c) { return c ? (uint64_t)c->grid : 0; }

} // extern "C"

// ---------------------------------------------------------------------------------------------------------------
// Layer pipeline, native transport.  No reference counterpart (the reference is single-device); the
// north_star asks for "layers optionally pipelined across the 8 GPUs of one node via RCCL send/recv over xGMI".
// The hop lives INSIDE the engine: ncclSend / ncclRecv are enqueued on the engine's own stream between the stage's
// graph launches, the greedy id travels last stage -> first stage as a device-to-device u64 straight into the control
// block the next launch reads, and the host never waits inside the loop (one synchronisation at the very end).
namespace {

int pipe_fail(Pipe *p, int rc, const char *what)
{
    return fail(RWKV_E_DEVICE, "%s: %s", what, (p && p->GetErrorString) ? p->GetErrorString(rc) : "RCCL error");
}
#define NCHK(expr) do { int r__ = (expr); if (r__ != 0) return pipe_fail(p, r__, #expr); } while (0)

int pipe_open(Pipe *p)
{
    if (p->lib) return 0;
    // Which RCCL: (1) RWKV_RCCL_LIB if set; (2) the copy the PROCESS HAS ALREADY LOADED -- a host that imported PyTorch-ROCm carries
    // torch/lib/librccl.so, built against the HIP runtime torch brought along, and the engine's streams and buffers live in that same
    // runtime: a second RCCL of another ROCm release beside it is a version mix nobody tests; (3) the system's, for a host without one.
    const char *env = getenv("RWKV_RCCL_LIB");
    if (env && env[0]) p->lib = dlopen(env, RTLD_NOW | RTLD_GLOBAL);
    if (!p->lib && !(env && env[0]))
        for (const char *n : {"librccl.so", "librccl.so.1"}) {
            p->lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL | RTLD_NOLOAD);
            if (p->lib) break;
        }
    if (!p->lib && !(env && env[0]))
        for (const char *n : {"librccl.so.1", "librccl.so"}) {
            p->lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
            if (p->lib) break;
        }
    if (!p->lib) return fail(RWKV_E_DEVICE, "cannot load %s (%s)", (env && env[0]) ? env : "librccl.so", dlerror());
    auto sym = [&](const char *n) { return dlsym(p->lib, n); };
    *(void **)&p->GetUniqueId = sym("ncclGetUniqueId");
    *(void **)&p->CommInitRank = sym("ncclCommInitRank");
    *(void **)&p->CommDestroy = sym("ncclCommDestroy");
    *(void **)&p->Send = sym("ncclSend");
    *(void **)&p->Recv = sym("ncclRecv");
    *(void **)&p->GroupStart = sym("ncclGroupStart");
    *(void **)&p->GroupEnd = sym("ncclGroupEnd");
    *(void **)&p->GetErrorString = sym("ncclGetErrorString");
    *(void **)&p->GetVersion = sym("ncclGetVersion");      // (optional: diagnostics only)
    if (!p->GetUniqueId || !p->CommInitRank || !p->Send || !p->Recv || !p->GroupStart || !p->GroupEnd)
        return fail(RWKV_E_DEVICE, "librccl.so lacks the point-to-point API");
    return 0;
}
constexpr int kNcclUint64 = 5, kNcclFloat64 = 8;

} // namespace

extern "C" {

// which RCCL the pipeline transport binds in this process (path of the shared object that holds ncclSend); loads it if need be.
// No GPU involved: a host can check the pairing before it builds a pipeline.
int rwkv_pipe_rccl_path(char *out, uint64_t cap)
{
    if (!out || cap == 0) return fail(RWKV_E_ARG, "NULL argument");
    static Pipe probe;
    int rc = pipe_open(&probe);
    if (rc) return rc;
    Dl_info info{};
    if (!dladdr(reinterpret_cast<void *>(probe.Send), &info) || !info.dli_fname) return fail(RWKV_E_DEVICE, "dladdr failed for ncclSend");
    snprintf(out, (size_t)cap, "%s", info.dli_fname);
    return 0;
}

// 128 opaque bytes (ncclUniqueId) made by ONE rank and handed to every rank of the pipeline out of band
int rwkv_pipe_unique_id(void *out128)
{
    if (!out128) return fail(RWKV_E_ARG, "NULL argument");
    static Pipe boot;
    Pipe *p = &boot;
    int rc = pipe_open(p);
    if (rc) return rc;
    Pipe::Id id;
    NCHK(p->GetUniqueId(&id));
    memcpy(out128, id.b, sizeof(id.b));
    return 0;
}

int rwkv_pipe_init(rwkv_ctx *c, const void *id128, int rank, int world)
{
    if (const int rc = guard(c, NEED_LOADED, id128)) return rc;
    if (world < 1 || rank < 0 || rank >= world) return fail(RWKV_E_ARG, "bad rank %d of %d", rank, world);
    if (c->pipe) return fail(RWKV_E_STATE, "pipeline transport already initialised");
    if ((rank == 0) != (c->l0 == 0) || (rank == world - 1) != (c->l1 == c->L))
        return fail(RWKV_E_ARG, "rank %d of %d does not match this context's layer range [%llu, %llu) of %llu", rank, world,
                    (unsigned long long)c->l0, (unsigned long long)c->l1, (unsigned long long)c->L);
    Pipe *p = new Pipe();
    int rc = pipe_open(p);
    if (rc) { delete p; return rc; }
    Pipe::Id id;
    memcpy(id.b, id128, sizeof(id.b));
    int r = p->CommInitRank(&p->comm, world, id, rank);
    if (r != 0) { rc = pipe_fail(p, r, "ncclCommInitRank"); delete p; return rc; }
    p->rank = rank; p->world = world;
    // every failure from here on gives the communicator back and leaves the context as it was (hop read from c->x)
    auto undo = [&](int code) {
        if (p->CommDestroy) (void)p->CommDestroy(p->comm);
        delete p;
        c->x_in = nullptr;
        return code;
    };
    if (rank > 0) {
        if ((rc = dalloc(c, &c->x_in, c->D))) return undo(rc);
        // the stage graphs captured at load time read the hop from c->x: rebuild them around x_in
        if ((rc = rebuild_graphs(c))) {
            c->x_in = nullptr;
            (void)rebuild_graphs(c);          // back to the graphs that read c->x (on failure: no graphs, eager launches)
            return undo(rc);
        }
    }
    // Every rank must cut a prompt into the SAME micro-batches (rwkv_pipe_prefill: rows per ncclSend / ncclRecv) and speak about the same
    // model: the values behind that are per-rank (RWKV_SEQ_ROWS in each process's environment, the max_ctx each context was loaded with),
    // so they are agreed here, once, over the communicator itself -- a ring pass of (min, max) per field, world - 1 hops, after which every
    // rank holds the same extremes and every rank fails the same way on a mismatch (a pipeline that disagrees would hang in its first
    // prefill hop, or corrupt the residual stream).
    {
        const uint64_t my_ch = !c->seq_ok ? 0 : (c->seq_rows > SEQ_T && c->maxT >= (uint64_t)SEQ_TM) ? (uint64_t)SEQ_TM : (c->maxT >= (uint64_t)SEQ_T ? (uint64_t)SEQ_T : 0);
        uint64_t mm[8] = {my_ch, my_ch, c->D, c->D, c->L, c->L, (uint64_t)world, (uint64_t)world};      // (min, max) pairs
        {   // (world == 1: one hop to SELF -- nothing to agree on, but it is the one ncclSend / ncclRecv group a single process can make on the
            //  real library: entry points, datatype codes, the group and the stream order are exercised before any pipeline depends on them)
            uint64_t *d = nullptr;
            if (hipMalloc(reinterpret_cast<void **>(&d), 16 * sizeof(uint64_t)) != hipSuccess) return undo(fail(RWKV_E_DEVICE, "rwkv_pipe_init: no device memory for the agreement round"));
            int r = 0;
            hipError_t e = hipSuccess;
            bool self_ok = true;
            const int hops = world > 1 ? world - 1 : 1;
            for (int hop = 0; hop < hops && !r && e == hipSuccess; hop++) {
                e = hipMemcpyAsync(d, mm, sizeof(mm), hipMemcpyHostToDevice, c->stream);
                if (e == hipSuccess) e = hipMemsetAsync(d + 8, 0xff, 8 * sizeof(uint64_t), c->stream);
                if (e != hipSuccess) break;
                r = p->GroupStart();
                if (!r) r = p->Send(d, 8, kNcclUint64, (rank + 1) % world, p->comm, c->stream);
                if (!r) r = p->Recv(d + 8, 8, kNcclUint64, (rank + world - 1) % world, p->comm, c->stream);
                const int r2 = p->GroupEnd();
                if (!r) r = r2;
                uint64_t got[8];
                if (!r) e = hipMemcpyAsync(got, d + 8, sizeof(got), hipMemcpyDeviceToHost, c->stream);
                if (!r && e == hipSuccess) e = hipStreamSynchronize(c->stream);
                if (!r && e == hipSuccess) {
                    if (world == 1) self_ok = memcmp(got, mm, sizeof(got)) == 0;
                    for (int k = 0; k < 8; k += 2) { mm[k] = std::min(mm[k], got[k]); mm[k + 1] = std::max(mm[k + 1], got[k + 1]); }
                }
            }
            (void)hipFree(d);
            if (r) { rc = pipe_fail(p, r, "agreement round of rwkv_pipe_init"); if (rank > 0) { c->x_in = nullptr; (void)rebuild_graphs(c); } return undo(rc); }
            if (e != hipSuccess) { rc = fail(RWKV_E_DEVICE, "agreement round of rwkv_pipe_init: %s", hipGetErrorString(e)); if (rank > 0) { c->x_in = nullptr; (void)rebuild_graphs(c); } return undo(rc); }
            if (!self_ok) return undo(fail(RWKV_E_DEVICE, "rwkv_pipe_init: a grouped ncclSend / ncclRecv of 8 x uint64 to this rank itself did not deliver what was sent"));
        }
        if (mm[0] != mm[1] || mm[2] != mm[3] || mm[4] != mm[5] || mm[6] != mm[7]) {
            rc = fail(RWKV_E_ARG, "the ranks of this pipeline disagree: prefill micro-batch rows %llu..%llu (RWKV_SEQ_ROWS / max_ctx differ between ranks; this rank: %llu), "
                                  "n_embed %llu..%llu, n_layers %llu..%llu, world %llu..%llu", (unsigned long long)mm[0], (unsigned long long)mm[1], (unsigned long long)my_ch,
                      (unsigned long long)mm[2], (unsigned long long)mm[3], (unsigned long long)mm[4], (unsigned long long)mm[5], (unsigned long long)mm[6], (unsigned long long)mm[7]);
            if (rank > 0) { c->x_in = nullptr; (void)rebuild_graphs(c); }
            return undo(rc);
        }
        p->ch = my_ch;
    }
    {   // what this rank's end of the transport is made of: for the first run on real xGMI to be diagnosable from its log / bench line
        int ver = -1;
        if (p->GetVersion) (void)p->GetVersion(&ver);
        Dl_info di{};
        const char *path = (dladdr(reinterpret_cast<void *>(p->Send), &di) && di.dli_fname) ? di.dli_fname : "?";
        char bus[64] = "?";
        (void)hipDeviceGetPCIBusId(bus, (int)sizeof(bus), c->device);
        hipDeviceProp_t prop{};
        (void)hipGetDeviceProperties(&prop, c->device);
        int rt = 0;
        (void)hipRuntimeGetVersion(&rt);
        char buf[1024];
        snprintf(buf, sizeof(buf), "{\"rank\": %d, \"world\": %d, \"layers\": [%llu, %llu], \"device\": %d, \"pci_bus_id\": \"%s\", \"arch\": \"%s\", \"cus\": %d, "
                                   "\"rccl_version\": %d, \"rccl_path\": \"%s\", \"hip_runtime\": %d, \"prefill_rows\": %llu, \"HSA_ENABLE_IPC_MODE_LEGACY\": \"%s\"}",
                 rank, world, (unsigned long long)c->l0, (unsigned long long)c->l1, c->device, bus, prop.gcnArchName, prop.multiProcessorCount, ver, path, rt,
                 (unsigned long long)p->ch, getenv("HSA_ENABLE_IPC_MODE_LEGACY") ? getenv("HSA_ENABLE_IPC_MODE_LEGACY") : "");
        p->info = buf;
        fprintf(stderr, "[rwkv_mi355x] pipeline transport up: %s\n", buf);
    }
    c->pipe = p;
    return 0;
}

// this rank's end of the pipeline transport as one JSON object (rank, world, layer range, device ordinal, PCI bus id, arch, RCCL
// version code and the path of the shared object that holds ncclSend, HIP runtime version, agreed prefill micro-batch rows)
int rwkv_pipe_info(rwkv_ctx *c, char *out, uint64_t cap)
{
    if (const int rc = guard(c, 0, out && cap)) return rc;
    if (!c->pipe) return fail(RWKV_E_STATE, "needs rwkv_pipe_init done");
    snprintf(out, (size_t)cap, "%s", c->pipe->info.c_str());
    return 0;
}

// Greedy decode of `world` independent streams (stream k starts from first_tokens[k], state slot k), n_steps tokens each,
// with the model's layers pipelined over the ranks: at tick t rank r works on item j = t - r (stream j % S, step j / S),
// so every GPU is busy once the pipe is full.  Per tick and rank, all on the engine stream:
//   control block of the item (pinned ring -> device)   -> ONE RCCL group { send x to r+1 | send the previous pick to
//   rank 0 (last rank) | recv x from r-1 | recv the fed-back id into the control block (rank 0) }   -> the stage's graph.
// first_tokens: [world] (read on rank 0).  picks: [world][n_steps] (written on the last rank; may be NULL elsewhere).
// n_streams < world leaves the other streams' slots of the schedule empty: n_streams = 1 is ONE stream through all the stages, i.e.
// the latency of single-stream decode on the pipeline, t_tok + (S - 1) hops + the fed-back id (SURVEY 8e "expected scaling").
// With rwkv_pipe_profile(ctx, 1) every tick whose RCCL group holds a receive is bracketed by an event pair (rwkv_pipe_hop_stats).
int rwkv_pipe_decode_streams(rwkv_ctx *c, const uint64_t *first_tokens, uint64_t n_steps, uint64_t n_streams, uint64_t *picks)
{
    if (const int rc = guard(c, NEED_LOADED | LAUNCHES)) return rc;
    if (!c->pipe) return fail(RWKV_E_STATE, "needs rwkv_pipe_init done");
    Pipe *p = c->pipe;
    const int S = p->world, rank = p->rank;
    const bool lastr = rank == S - 1;
    const uint64_t n_items = (uint64_t)S * n_steps;
    if (n_streams == 0 || n_streams > (uint64_t)S) return fail(RWKV_E_ARG, "n_streams must be in 1..world");
    if (n_steps == 0 || n_items > c->gen_cap) return fail(RWKV_E_ARG, "world * n_steps must be in 1..%u", c->gen_cap);
    if ((uint64_t)S > c->maxT) return fail(RWKV_E_ARG, "needs max_ctx >= %d state slots (one per stream in flight)", S);
    if (rank == 0 && !first_tokens) return fail(RWKV_E_ARG, "rank 0 needs first_tokens");
    if (lastr && !picks) return fail(RWKV_E_ARG, "the last rank needs picks");
    // A bad id must not strand the other ranks in their ncclRecv: rank 0 runs the schedule with id 0 in its place and reports
    // the error when the schedule has drained (the argument checks above depend only on values every rank shares).
    bool bad_id = false;
    if (rank == 0)
        for (int k = 0; k < (int)n_streams; k++) bad_id = bad_id || first_tokens[k] >= RWKV_VOCAB;
    if (c->pipe_ring_cap < n_items) {
        if (c->pipe_ring) { HIPCHK(hipStreamSynchronize(c->stream)); (void)hipHostFree(c->pipe_ring); c->pipe_ring = nullptr; c->pipe_ring_cap = 0; }
        HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&c->pipe_ring), sizeof(Ctl) * n_items, hipHostMallocDefault));
        c->pipe_ring_cap = n_items;
    }
    Ctl *ring = c->pipe_ring;
    for (uint64_t j = 0; j < n_items; j++) {
        const uint64_t stream = j % S, step = j / S;
        ring[j].token = (rank == 0 && step == 0 && stream < n_streams) ? (first_tokens[stream] < RWKV_VOCAB ? first_tokens[stream] : 0) : 0;
        ring[j].slot = (unsigned)stream; ring[j].out_row = (unsigned)stream; ring[j].step = (unsigned)j; ring[j].pad = 0;
    }
    auto active = [&](uint64_t j) { return j % (uint64_t)S < n_streams; };
    auto has_work = [&](int r, uint64_t t) { return t >= (uint64_t)r && t - r < n_items && active(t - r); };
    int rc = 0;
    size_t hop_n = 0;
    for (uint64_t tick = 0; tick < n_items + S - 1 && !rc; tick++) {
        const bool work = has_work(rank, tick);
        const bool feedback = tick >= (uint64_t)S && tick < n_items && active(tick);   // stage 0 starts a step >= 1: its token is the last stage's pick
        const uint64_t j = tick - rank;
        if (work && hipMemcpyAsync(c->ctl, &ring[j], sizeof(Ctl), hipMemcpyHostToDevice, c->stream) != hipSuccess) { rc = fail(RWKV_E_DEVICE, "control block copy failed"); break; }
        bool timed = c->pipe_prof && S > 1 && ((rank > 0 && work) || (rank == 0 && feedback)) && hop_n < rwkv_ctx::HOP_EV;
        if (timed) {      // (a failure here only drops the measurement: the schedule must go on, the peers are waiting)
            if (!c->hop_ev[2 * hop_n] && (hipEventCreate(&c->hop_ev[2 * hop_n]) != hipSuccess || hipEventCreate(&c->hop_ev[2 * hop_n + 1]) != hipSuccess)) timed = false;
            if (timed && hipEventRecord(c->hop_ev[2 * hop_n], c->stream) != hipSuccess) timed = false;
        }
        if (S > 1) {
            int r = p->GroupStart();
            if (!r && rank < S - 1 && has_work(rank + 1, tick)) r = p->Send(c->x, c->D, kNcclFloat64, rank + 1, p->comm, c->stream);
            if (!r && lastr && feedback) r = p->Send(c->gen + (tick - S), 1, kNcclUint64, 0, p->comm, c->stream);   // item tick - S: produced here one tick ago
            if (!r && rank > 0 && work) r = p->Recv(c->x_in, c->D, kNcclFloat64, rank - 1, p->comm, c->stream);
            if (!r && rank == 0 && feedback) r = p->Recv(&c->ctl->token, 1, kNcclUint64, S - 1, p->comm, c->stream);
            const int r2 = p->GroupEnd();
            if (r || r2) { rc = pipe_fail(p, r ? r : r2, "RCCL hop"); break; }
            if (timed && hipEventRecord(c->hop_ev[2 * hop_n + 1], c->stream) == hipSuccess) hop_n++;
        } else if (feedback) {
            // one stage: the pick of the previous step is already in ctl->token ... but the control block was just overwritten
            HIPCHK(hipMemcpyAsync(&c->ctl->token, c->gen + (j - 1), sizeof(uint64_t), hipMemcpyDeviceToDevice, c->stream));
        }
        if (work) rc = run_token(c, lastr);
    }
    hipError_t e = hipStreamSynchronize(c->stream);
    if (!rc && e != hipSuccess) rc = fail(RWKV_E_DEVICE, "pipeline decode: %s", hipGetErrorString(e));
    if (!rc && lastr) {
        std::vector<uint64_t> g(n_items);
        if (hipMemcpy(g.data(), c->gen, n_items * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(RWKV_E_DEVICE, "copy of the picks failed");
        else for (uint64_t j = 0; j < n_items; j++) picks[(j % S) * n_steps + j / S] = active(j) ? g[j] : 0;     // (rows of streams that did not run: zero)
    }
    { const int dc = device_check(c); if (!rc) rc = dc; }      // always consumed: a code raised here must not surface from a later call
    if (!rc && c->pipe_prof) {
        double sum = 0.0, mn = 1e30, mx = 0.0;
        for (size_t i = 0; i < hop_n; i++) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, c->hop_ev[2 * i], c->hop_ev[2 * i + 1]) != hipSuccess) continue;
            sum += ms; mn = std::min(mn, (double)ms); mx = std::max(mx, (double)ms);
        }
        c->hop_stats[0] = (double)hop_n; c->hop_stats[1] = hop_n ? 1e3 * sum / hop_n : 0.0; c->hop_stats[2] = hop_n ? 1e3 * mn : 0.0; c->hop_stats[3] = 1e3 * mx;
    }
    if (!rc && bad_id) rc = fail(RWKV_E_ARG, "token id out of range (the schedule ran with id 0 in its place)");
    return rc;
}

// ---- 2 x world streams in flight on TWO communicators: the hop under the compute -------------------------------------------------------
// rwkv_pipe_decode* above runs hop and stage strictly one after the other on the engine's stream: every tick costs t_hop + t_stage.  Here a
// rank keeps TWO independent copies of that schedule going -- the streams of even index on communicator 0 and HIP stream cs[0], those of odd
// index on communicator 1 and cs[1], each with its own hop buffers -- and ONE compute stream (the engine's) that alternates between them:
// while the stage works on parity 0's item, parity 1's RCCL group {send the previous result | recv the next input} is in flight, and vice
// versa.  A tick costs max(t_stage, t_hop) once both are primed.  Two communicators, because operations of one communicator are serialised
// in the order they were enqueued whatever stream they are on: a receive that waits for its peer would hold the other parity's send behind
// it.  Each sub-schedule is the tick schedule of rwkv_pipe_decode_streams (same group composition, same deadlock argument); events order
// the comm streams against the compute stream: ev_rx[k] (the group's receives have landed) and ev_cp[k] (the stage's output is in
// xout[k], xin[k] has been consumed).  Results are those of 2 x world independent greedy decodes (stream g on state slot g).
namespace {
// streams, hop buffers and events of the two-communicator schedule (not the communicator itself): idempotent, also the clean-up of a set-up
// that failed half way
void pipe_dual_teardown(Pipe *p)
{
    for (int k = 0; k < 2; k++) {
        if (p->cs[k]) { (void)hipStreamSynchronize(p->cs[k]); (void)hipStreamDestroy(p->cs[k]); p->cs[k] = nullptr; }
        if (p->xin[k]) { (void)hipFree(p->xin[k]); p->xin[k] = nullptr; }
        if (p->xout[k]) { (void)hipFree(p->xout[k]); p->xout[k] = nullptr; }
        if (p->idbuf[k]) { (void)hipFree(p->idbuf[k]); p->idbuf[k] = nullptr; }
        if (p->ev_rx[k]) { (void)hipEventDestroy(p->ev_rx[k]); p->ev_rx[k] = nullptr; }
        if (p->ev_cp[k]) { (void)hipEventDestroy(p->ev_cp[k]); p->ev_cp[k] = nullptr; }
    }
    p->dual_ready = false;
}
// Re-entrant: `dual_ready` is set only when every resource AND the second communicator exist; a call that fails half way
// frees what it made and the next call starts over.  The id exchange always completes on every rank: if rank 0 cannot make an id it sends
// an all-zero one, which every rank (rank 0 included) treats as the failure it is -- nobody is left blocked in a receive.
int pipe_dual_setup(rwkv_ctx *c)
{
    Pipe *p = c->pipe;
    if (p->dual_ready) return 0;
    pipe_dual_teardown(p);
    const int S = p->world, rank = p->rank;
    if (S > 1 && !p->comm2) {
        // the second communicator's id is made by rank 0 and travels over the first one (16 x u64)
        unsigned long long *d = nullptr;
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&d), sizeof(Pipe::Id)));
        Pipe::Id id;
        memset(&id, 0, sizeof(id));
        int r = 0, r_id = 0;
        if (rank == 0) {
            r_id = p->GetUniqueId(&id);
            if (r_id) memset(&id, 0, sizeof(id));               // the peers learn of the failure from the id itself
            if (hipMemcpyAsync(d, id.b, sizeof(id.b), hipMemcpyHostToDevice, c->stream) != hipSuccess) r = -1;
            if (!r) {
                r = p->GroupStart();
                for (int q = 1; q < S && !r; q++) r = p->Send(d, sizeof(id.b) / 8, kNcclUint64, q, p->comm, c->stream);
                const int r2 = p->GroupEnd();
                if (!r) r = r2;
            }
        } else {
            r = p->Recv(d, sizeof(id.b) / 8, kNcclUint64, 0, p->comm, c->stream);
            if (!r && hipMemcpyAsync(id.b, d, sizeof(id.b), hipMemcpyDeviceToHost, c->stream) != hipSuccess) r = -1;
        }
        const hipError_t e = hipStreamSynchronize(c->stream);
        (void)hipFree(d);
        if (r_id) return pipe_fail(p, r_id, "ncclGetUniqueId (second communicator)");
        if (r) return pipe_fail(p, r > 0 ? r : 1, "exchange of the second communicator's id");
        HIPCHK(e);
        bool zero = true;
        for (size_t q = 0; q < sizeof(id.b); q++) zero = zero && id.b[q] == 0;
        if (zero) return fail(RWKV_E_DEVICE, "rank 0 could not make the second communicator's id (it sent the all-zero id)");
        r = p->CommInitRank(&p->comm2, S, id, rank);
        if (r) { p->comm2 = nullptr; return pipe_fail(p, r, "ncclCommInitRank (second communicator)"); }
    }
    auto make = [&]() -> int {
        for (int k = 0; k < 2; k++) {
            HIPCHK(hipStreamCreateWithFlags(&p->cs[k], hipStreamNonBlocking));
            HIPCHK(hipMalloc(reinterpret_cast<void **>(&p->xin[k]), c->D * sizeof(double)));
            HIPCHK(hipMalloc(reinterpret_cast<void **>(&p->xout[k]), c->D * sizeof(double)));
            HIPCHK(hipMalloc(reinterpret_cast<void **>(&p->idbuf[k]), 64));
            HIPCHK(hipEventCreateWithFlags(&p->ev_rx[k], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&p->ev_cp[k], hipEventDisableTiming));
        }
        return 0;
    };
    const int rm = make();
    if (rm) { pipe_dual_teardown(p); return rm; }
    p->dual_ready = true;
    return 0;
}
} // namespace

// first_tokens: [2 * world] (read on rank 0); picks: [2 * world][n_steps] (written on the last rank).  Needs max_ctx >= 2 * world state slots.
int rwkv_pipe_decode_dual(rwkv_ctx *c, const uint64_t *first_tokens, uint64_t n_steps, uint64_t *picks)
{
    if (const int rc = guard(c, NEED_LOADED | LAUNCHES)) return rc;
    if (!c->pipe) return fail(RWKV_E_STATE, "needs rwkv_pipe_init done");
    Pipe *p = c->pipe;
    const int S = p->world, rank = p->rank;
    const bool lastr = rank == S - 1;
    const uint64_t n_sub = (uint64_t)S * n_steps;             // items of ONE sub-schedule
    if (n_steps == 0 || 2 * n_sub > c->gen_cap) return fail(RWKV_E_ARG, "2 * world * n_steps must be in 1..%u", c->gen_cap);
    if ((uint64_t)(2 * S) > c->maxT) return fail(RWKV_E_ARG, "needs max_ctx >= %d state slots (two streams per stage in flight)", 2 * S);
    if (rank == 0 && !first_tokens) return fail(RWKV_E_ARG, "rank 0 needs first_tokens");
    if (lastr && !picks) return fail(RWKV_E_ARG, "the last rank needs picks");
    bool bad_id = false;
    if (rank == 0)
        for (int g = 0; g < 2 * S; g++) bad_id = bad_id || first_tokens[g] >= RWKV_VOCAB;
    { const int rs = pipe_dual_setup(c); if (rs) return rs; }
    if (c->pipe_ring_cap < 2 * n_sub) {
        if (c->pipe_ring) { HIPCHK(hipStreamSynchronize(c->stream)); (void)hipHostFree(c->pipe_ring); c->pipe_ring = nullptr; c->pipe_ring_cap = 0; }
        HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&c->pipe_ring), sizeof(Ctl) * 2 * n_sub, hipHostMallocDefault));
        c->pipe_ring_cap = 2 * n_sub;
    }
    // item (k, i): sub-schedule k, sub-item i -> global stream g = 2 (i % S) + k, step i / S, id J = 2 i + k (its slot in the pick list)
    Ctl *ring = c->pipe_ring;
    for (uint64_t i = 0; i < n_sub; i++)
        for (int k = 0; k < 2; k++) {
            const uint64_t J = 2 * i + k, g = 2 * (i % S) + k, step = i / S;
            ring[J].token = (rank == 0 && step == 0) ? (first_tokens[g] < RWKV_VOCAB ? first_tokens[g] : 0) : 0;
            ring[J].slot = (unsigned)g; ring[J].out_row = (unsigned)g; ring[J].step = (unsigned)J; ring[J].pad = 0;
        }
    auto has_work = [&](int r, uint64_t t) { return t >= (uint64_t)r && t - r < n_sub; };
    int rc = 0;
    // everything enqueued so far on the engine's stream precedes the comm streams' first operation
    for (int k = 0; k < 2 && !rc; k++) {
        if (hipEventRecord(p->ev_cp[k], c->stream) != hipSuccess || hipStreamWaitEvent(p->cs[k], p->ev_cp[k], 0) != hipSuccess) rc = fail(RWKV_E_DEVICE, "event setup failed");
    }
    for (uint64_t tick = 0; tick < n_sub + S - 1 && !rc; tick++) {
        const bool work = has_work(rank, tick);
        const bool feedback = tick >= (uint64_t)S && tick < n_sub;       // stage 0 starts a step >= 1: its token is the last stage's pick
        const uint64_t i = tick - rank;
        // ---- the hops of both parities, each on its own communicator and stream ----
        for (int k = 0; k < 2 && !rc && S > 1; k++) {
            void *comm = k == 0 ? p->comm : p->comm2;
            hipStream_t cs = p->cs[k];
            if (tick > 0 && has_work(rank, tick - 1) && hipStreamWaitEvent(cs, p->ev_cp[k], 0) != hipSuccess) { rc = fail(RWKV_E_DEVICE, "event wait failed"); break; }
            int r = p->GroupStart();
            if (!r && rank < S - 1 && has_work(rank + 1, tick)) r = p->Send(p->xout[k], c->D, kNcclFloat64, rank + 1, comm, cs);
            if (!r && lastr && feedback) r = p->Send(c->gen + (2 * (tick - S) + k), 1, kNcclUint64, 0, comm, cs);      // sub-item tick - S: finished here one tick ago
            if (!r && rank > 0 && work) r = p->Recv(p->xin[k], c->D, kNcclFloat64, rank - 1, comm, cs);
            if (!r && rank == 0 && feedback) r = p->Recv(p->idbuf[k], 1, kNcclUint64, S - 1, comm, cs);
            const int r2 = p->GroupEnd();
            if (r || r2) { rc = pipe_fail(p, r ? r : r2, "RCCL hop"); break; }
            if (hipEventRecord(p->ev_rx[k], cs) != hipSuccess) rc = fail(RWKV_E_DEVICE, "event record failed");
        }
        // ---- the stage, parity 0 then parity 1, on the engine's stream ----
        for (int k = 0; k < 2 && !rc && work; k++) {
            const uint64_t J = 2 * i + k;
            if (S > 1 && hipStreamWaitEvent(c->stream, p->ev_rx[k], 0) != hipSuccess) { rc = fail(RWKV_E_DEVICE, "event wait failed"); break; }
            if (hipMemcpyAsync(c->ctl, &ring[J], sizeof(Ctl), hipMemcpyHostToDevice, c->stream) != hipSuccess) { rc = fail(RWKV_E_DEVICE, "control block copy failed"); break; }
            if (feedback && rank == 0) {
                const void *src = S > 1 ? static_cast<const void *>(p->idbuf[k]) : static_cast<const void *>(c->gen + (J - 2 * (uint64_t)S));
                if (hipMemcpyAsync(&c->ctl->token, src, sizeof(uint64_t), hipMemcpyDeviceToDevice, c->stream) != hipSuccess) { rc = fail(RWKV_E_DEVICE, "id copy failed"); break; }
            }
            if (rank > 0 && hipMemcpyAsync(c->x_in, p->xin[k], c->D * sizeof(double), hipMemcpyDeviceToDevice, c->stream) != hipSuccess) { rc = fail(RWKV_E_DEVICE, "hop copy failed"); break; }
            rc = run_token(c, lastr);
            if (!rc && rank < S - 1 && hipMemcpyAsync(p->xout[k], c->x, c->D * sizeof(double), hipMemcpyDeviceToDevice, c->stream) != hipSuccess) rc = fail(RWKV_E_DEVICE, "hop copy failed");
            if (!rc && hipEventRecord(p->ev_cp[k], c->stream) != hipSuccess) rc = fail(RWKV_E_DEVICE, "event record failed");
        }
    }
    hipError_t e = hipStreamSynchronize(c->stream);
    for (int k = 0; k < 2; k++) { const hipError_t e2 = hipStreamSynchronize(p->cs[k]); if (e == hipSuccess) e = e2; }
    if (!rc && e != hipSuccess) rc = fail(RWKV_E_DEVICE, "pipeline decode (dual): %s", hipGetErrorString(e));
    if (!rc && lastr) {
        std::vector<uint64_t> g(2 * n_sub);
        if (hipMemcpy(g.data(), c->gen, 2 * n_sub * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(RWKV_E_DEVICE, "copy of the picks failed");
        else
            for (uint64_t i = 0; i < n_sub; i++)
                for (int k = 0; k < 2; k++) picks[(2 * (i % S) + k) * n_steps + i / S] = g[2 * i + k];
    }
    { const int dc = device_check(c); if (!rc) rc = dc; }
    if (!rc && bad_id) rc = fail(RWKV_E_ARG, "token id out of range (the schedule ran with id 0 in its place)");
    return rc;
}

int rwkv_pipe_decode(rwkv_ctx *c, const uint64_t *first_tokens, uint64_t n_steps, uint64_t *picks)
{
    if (!c || !c->pipe) return fail(RWKV_E_STATE, "needs a loaded context with rwkv_pipe_init done");
    return rwkv_pipe_decode_streams(c, first_tokens, n_steps, (uint64_t)c->pipe->world, picks);
}
// hop timing (off by default: two event records per tick): out4 = {ticks measured, mean, min, max us} of the span, on this rank's
// stream, from just before the tick's RCCL group {send | recv} to just behind it, over the ticks of the last rwkv_pipe_decode* call
// whose group held a receive.  The MIN is the hop itself (the peer's data was waiting); the mean includes waiting for the peer.
int rwkv_pipe_profile(rwkv_ctx *c, int on)
{
    if (const int rc = guard(c, 0)) return rc;
    c->pipe_prof = on != 0;
    return 0;
}
int rwkv_pipe_hop_stats(rwkv_ctx *c, double *out4)
{
    if (const int rc = guard(c, 0, out4)) return rc;
    for (int k = 0; k < 4; k++) out4[k] = c->hop_stats[k];
    return 0;
}

// ---- prompt chunks on a pipeline stage -----------------------------------------------------------------------
// One chunk (n <= 32 tokens of ONE sequence, GPT mode) through this context's layers on the MFMA path; the chunk's
// residual stream sits in buffer `buf` (0/1): stage 0 fills it from `tokens`, a later stage expects the previous stage's
// output there (rwkv_xseq_device / rwkv_xseq_copy, or the RCCL recv of rwkv_pipe_prefill).  Asynchronous.
int rwkv_stage_chunk(rwkv_ctx *c, const uint64_t *tokens, uint64_t n, uint64_t row0, int buf)
{
    if (const int rc = guard(c, NEED_SEQ)) return rc;      // (not LAUNCHES: asynchronous -- what the device error word holds is rwkv_sync's to report)
    if (n == 0 || n > (uint64_t)SEQ_TM || row0 + n > c->maxT || (buf != 0 && buf != 1)) return fail(RWKV_E_ARG, "bad chunk (n %llu <= 64, row0 %llu, buf %d)", (unsigned long long)n, (unsigned long long)row0, buf);
    if (c->l0 == 0) {
        if (!tokens) return fail(RWKV_E_ARG, "stage 0 needs the token ids");
        if (const int rc = check_ids(tokens, n, "token")) return rc;
    }
    return enqueue_whole(c, tokens, (int)n, row0, buf);
}
double *rwkv_xseq_device(rwkv_ctx *c, int buf) { return (c && (buf == 0 || buf == 1)) ? c->sq_x[buf] : nullptr; }
int rwkv_sync(rwkv_ctx *c)
{
    if (const int rc = guard(c, 0)) return rc;
    return finish(c, 0);
}
// hand a chunk's residual stream from one stage context to the next ON THE SAME DEVICE (virtual stages: tests, and
// several stages per GPU); ordered behind src's work, and dst's later work is ordered behind the copy
int rwkv_xseq_copy(rwkv_ctx *dst, int dbuf, rwkv_ctx *src, int sbuf, uint64_t rows)
{
    if (!dst || !src || !dst->seq_ok || !src->seq_ok || dst->D != src->D || rows > (uint64_t)SEQ_TM) return fail(RWKV_E_ARG, "bad copy");
    HIPCHK(hipSetDevice(src->device));
    // Stream-ordered, no host wait: dst's stream waits for what src's stream has enqueued so far (the chunk that filled the
    // buffer), copies, and src's stream waits for the copy before it may overwrite the buffer -- so two stages on one GPU run
    // CONCURRENTLY, stage s on chunk c while stage s-1 is on chunk c+1 (each kernel's start-up and tail under the other's stream).
    if (!dst->xs_ev[0]) {
        HIPCHK(hipEventCreateWithFlags(&dst->xs_ev[0], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&dst->xs_ev[1], hipEventDisableTiming));
    }
    HIPCHK(hipEventRecord(dst->xs_ev[0], src->stream));
    HIPCHK(hipStreamWaitEvent(dst->stream, dst->xs_ev[0], 0));
    HIPCHK(hipMemcpyAsync(dst->sq_x[dbuf & 1], src->sq_x[sbuf & 1], rows * src->D * sizeof(double), hipMemcpyDeviceToDevice, dst->stream));
    HIPCHK(hipEventRecord(dst->xs_ev[1], dst->stream));
    HIPCHK(hipStreamWaitEvent(src->stream, dst->xs_ev[1], 0));
    return 0;
}

// Pipelined prompt ingestion (RWKV::loadContext, rwkv.h:395-413, across the stages): the prompt's 32-token chunks are
// micro-batches, rank r works on chunk t - r at tick t.  Per tick: ONE RCCL group { send the finished chunk's residual
// stream [rows][D] to r+1 | recv the next chunk's from r-1 into the other buffer }, then the chunk through this stage's
// layers.  tokens: the whole prompt (read on rank 0; other ranks only need n_tokens).  Every chunk writes its logits to rows
// [0, rows) of the last stage's logits buffer (position % 32): after the call the buffer holds the LAST chunk's rows, which is
// what RWKV::loadContext's caller reads; returns after the stage's stream has drained.
int rwkv_pipe_prefill(rwkv_ctx *c, const uint64_t *tokens, uint64_t n_tokens)
{
    if (const int rc = guard(c, NEED_SEQ | LAUNCHES)) return rc;
    if (!c->pipe) return fail(RWKV_E_STATE, "needs rwkv_pipe_init done");
    if (c->maxT < (uint64_t)SEQ_T) return fail(RWKV_E_ARG, "needs max_ctx >= %d", SEQ_T);
    Pipe *p = c->pipe;
    const int S = p->world, rank = p->rank;
    if (n_tokens == 0 || (rank == 0 && !tokens)) return fail(RWKV_E_ARG, "empty prompt");
    // k_seq_embed indexes the table with the id: validate the whole prompt on rank 0.  A bad id must not strand the other ranks in
    // their ncclRecv, so the schedule runs with id 0 in its place and the error is reported once it has drained.
    std::vector<uint64_t> clean;
    bool bad_id = false;
    if (rank == 0) {
        for (uint64_t t = 0; t < n_tokens; t++) bad_id = bad_id || tokens[t] >= RWKV_VOCAB;
        if (bad_id) {
            clean.assign(tokens, tokens + n_tokens);
            for (auto &t : clean) if (t >= RWKV_VOCAB) t = 0;
            tokens = clean.data();
        }
    }
    // micro-batch = one weight pass of the stage: 64 rows (two halves per weight fragment) where the contexts allow, else 32
    const uint64_t CH = p->ch;       // agreed by all ranks in rwkv_pipe_init (a per-rank value here could differ between ranks: hang or corruption)
    if (CH == 0) return fail(RWKV_E_STATE, "chunked path not available on every rank (load with max_ctx >= 32)");
    const uint64_t n_chunks = (n_tokens + CH - 1) / CH;
    auto rows_of = [&](uint64_t ci) { return ci + 1 < n_chunks ? CH : n_tokens - ci * CH; };
    auto has_work = [&](int r, uint64_t t) { return t >= (uint64_t)r && t - r < n_chunks; };
    int rc = 0;
    for (uint64_t tick = 0; tick < n_chunks + S - 1 && !rc; tick++) {
        const bool work = has_work(rank, tick);
        const uint64_t ci = tick - rank;
        if (S > 1) {
            int r = p->GroupStart();
            if (!r && rank < S - 1 && has_work(rank + 1, tick)) r = p->Send(c->sq_x[(ci - 1) & 1], rows_of(ci - 1) * c->D, kNcclFloat64, rank + 1, p->comm, c->stream);
            if (!r && rank > 0 && work) r = p->Recv(c->sq_x[ci & 1], rows_of(ci) * c->D, kNcclFloat64, rank - 1, p->comm, c->stream);
            const int r2 = p->GroupEnd();
            if (r || r2) { rc = pipe_fail(p, r ? r : r2, "RCCL hop"); break; }
        }
        if (work) rc = enqueue_whole(c, rank == 0 ? tokens + ci * CH : nullptr, (int)rows_of(ci), 0, (int)(ci & 1));
    }
    hipError_t e = hipStreamSynchronize(c->stream);
    if (!rc && e != hipSuccess) rc = fail(RWKV_E_DEVICE, "pipeline prefill: %s", hipGetErrorString(e));
    { const int dc = device_check(c); if (!rc) rc = dc; }
    if (!rc && bad_id) rc = fail(RWKV_E_ARG, "token id out of range (the schedule ran with id 0 in its place)");
    return rc;
}

void rwkv_pipe_free(rwkv_ctx *c)
{
    if (!c || !c->pipe) return;
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    pipe_dual_teardown(c->pipe);
    if (c->pipe->comm2 && c->pipe->CommDestroy) (void)c->pipe->CommDestroy(c->pipe->comm2);
    if (c->pipe->comm && c->pipe->CommDestroy) (void)c->pipe->CommDestroy(c->pipe->comm);
    delete c->pipe;
    c->pipe = nullptr;
    if (c->pipe_ring) { (void)hipHostFree(c->pipe_ring); c->pipe_ring = nullptr; c->pipe_ring_cap = 0; }
    // a later rank read the hop from x_in: any other transport (rwkv_stage_forward callers write rwkv_x_device()) needs the
    // graphs back on c->x, or it would compute on a stale x_in
    if (c->x_in) { c->x_in = nullptr; (void)rebuild_graphs(c); }
}

// Device pointer behind tensor slot `slot` of the reference's `tensors[]` table (rwkv.h:248, enums/enum.h:7-55) where the
// engine keeps that tensor in FILE layout: the f32/f64 vectors, the five state arrays, x and the logits buffer (BUFFER2).
// The uint8 matrices are re-tiled at load (no file-layout copy stays on the device) and the pure scratch slots have no
// counterpart: NULL.  EMBED is a DEVICE pointer here (the reference keeps the table on the host, rwkv.cu:683-684).
void *rwkv_tensor_device(rwkv_ctx *c, int slot)
{
    if (!c || !c->loaded) return nullptr;
    switch (slot) {
    case X: return c->x;
    case EMBED: return c->embed;
    case LAYERNORMS: return c->ln;
    case STATEXY: return c->state[0];
    case STATEAA: return c->state[1];
    case STATEBB: return c->state[2];
    case STATEPP: return c->state[3];
    case STATEDD: return c->state[4];
    case BUFFER2: return c->logits;
    case MIXK: return c->mixk;
    case MIXV: return c->mixv;
    case MIXR: return c->mixr;
    case KR: return c->kr;
    case VR: return c->vr;
    case RR: return c->rr;
    case O1: return c->o1;
    case O2: return c->o2;
    case O3: return c->o3;
    case ATTOUTR: return c->attr;
    case ATTOUTO: return c->atto;
    case FFNMIXK: return c->fmixk;
    case FFNMIXV: return c->fmixr;
    case FFNKR: return c->fkr;
    case FFNVR: return c->fvr;
    case FFNRR: return c->frr;
    case FFNKO: return c->fko;
    case FFNVO: return c->fvo;
    case FFNRO: return c->fro;
    case HEADR: return c->headr;
    case HEADO: return c->heado;
    default: return nullptr;
    }
}

} // extern "C"
