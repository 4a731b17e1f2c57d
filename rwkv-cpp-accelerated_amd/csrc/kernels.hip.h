// kernels.hip.h -- gfx950 (MI355X / CDNA4) device code of the RWKV-v4 uint8 engine.
//
// One token = 4 launches per layer + embed + head (+ argmax), replacing the ~28 stream
// operations per layer of the reference driver (rwkv.cu:528-581):
//
//   k_first       rwkv.cu:513-524   embedding row gather (device-resident table) + ln0; opens ln1 site
//   k_att         rwkv.cu:535-545   ln1 + token-shift mix + K/V/R dequant-GEMV + WKV recurrence
//   k_attout      rwkv.cu:548-553   att_out dequant-GEMV + residual; commits state xy; opens ln2 site
//   k_ffn_rk      rwkv.cu:557-573   ln2 + mix + ffn_r GEMV + sigmoid, ffn_k GEMV + relu^2
//   k_ffnv        rwkv.cu:574-577   ffn_v dequant-GEMV, x += v * sigmoid(r); commits state dd; opens next site
//   k_head        rwkv.cu:585-589   ln_out + head dequant-GEMV -> logits (+ per-block argmax)
//
// Design (DESIGN.md has the long form and the measurements behind each choice):
//  * The uint8 matrices are re-tiled at load into ROW-PER-OUTPUT order (w_t[k][j], j contiguous),
//    so one wavefront owns whole output rows: each lane streams 16-byte pieces of the row with
//    non-temporal global_load_dwordx4 (1 KiB per wave-instruction, every 128-B line used once)
//    and the row is finished by a 64-lane shuffle reduction.  No float atomics, no pre-zeroed
//    accumulators, no cross-workgroup reduction: results are deterministic and every epilogue
//    (WKV, sigmoid, relu^2, residual) fuses into the kernel that finished the row.
//  * sum_j x_j (u_jk r_j + o_j) = sum_j (x_j r_j) u_jk + sum_j x_j o_j.  The first term is an
//    integer contraction: the pre-scaled activation vector is quantised ONCE per workgroup to
//    23-bit fixed point (3 unsigned byte limbs, scale = max|.|/4194000) and staged in LDS, and
//    the u8 x u8 products run on v_dot4_u32_u8 (4 MACs per lane-instruction, exact u32
//    accumulation, no byte->float converts).  Measured on MI355X the f32 formulation
//    (v_cvt_f32_ubyteN + v_fma_f32 per weight byte) cost as much VALU time as the HBM stream
//    itself; the limb form needs 12 instructions per 16 weight bytes instead of 32 and its
//    rounding error (<= 1.2e-7 max|x| per element) is below that of an f32 FMA chain.  The offset term is
//    one scalar per vector.
//  * Every GEMV needs its complete input vector in every workgroup.  The LayerNorm / token-shift
//    work is split by ownership ("LayerNorm sites" below): the kernel that owns rows of x emits the
//    state-dependent part and per-workgroup partial sums, the consumer needs one reduction round
//    and one multiply-add per element before it can stage the vector.
//  * Grid = one 512-thread workgroup per CU (8 waves); each wave keeps R*S x 16 B loads in flight
//    and refills a step's registers with the next row group as soon as the step is consumed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rwkvk {

constexpr int NT = 512;          // threads per workgroup
constexpr int NW = NT / 64;      // wavefronts per workgroup
constexpr int RED_BYTES = 1024;  // LDS scratch for workgroup reductions
// rows [block_lo(n), block_hi(n)) of n belong to this workgroup: floor(b n / blocks) in 32-bit arithmetic (b n < 2^32 for every
// use: blocks <= 512, n <= 65536).  As a 64-bit expression it compiled to two ~130-instruction scalar divisions at the head of
// every wave, in front of the kernel-argument loads -- half a microsecond of every launch before the prologue's first request.
// Kernel arguments the prologue needs, fetched with the kernel's FIRST scalar loads: hipcc sinks an argument's s_load into the block
// that uses it, so the prologue waves paid a second and a third scalar-cache round trip (the role branch, then the site's
// pointers) before their first request to memory.
#define RWKV_ARGS_NOW(...) asm volatile("" ::RWKV_ARGS_S(__VA_ARGS__))
#define RWKV_ARGS_S(...) RWKV_ARGS_PICK(__VA_ARGS__, RWKV_A8, RWKV_A7, RWKV_A6, RWKV_A5, RWKV_A4, RWKV_A3, RWKV_A2, RWKV_A1)(__VA_ARGS__)
#define RWKV_ARGS_PICK(a, b, c, d, e, f, g, h, N, ...) N
#define RWKV_A1(a) "s"(a)
#define RWKV_A2(a, ...) "s"(a), RWKV_A1(__VA_ARGS__)
#define RWKV_A3(a, ...) "s"(a), RWKV_A2(__VA_ARGS__)
#define RWKV_A4(a, ...) "s"(a), RWKV_A3(__VA_ARGS__)
#define RWKV_A5(a, ...) "s"(a), RWKV_A4(__VA_ARGS__)
#define RWKV_A6(a, ...) "s"(a), RWKV_A5(__VA_ARGS__)
#define RWKV_A7(a, ...) "s"(a), RWKV_A6(__VA_ARGS__)
#define RWKV_A8(a, ...) "s"(a), RWKV_A7(__VA_ARGS__)
// the wave's index in its workgroup as a wave-UNIFORM value.  (threadIdx.x >> 6 is uniform in fact but "divergent" to the compiler: a role
// branch on it -- loader / prologue / consumer -- is then compiled as exec-masked straight-line code, every wave walks through every
// role's blocks, and hipcc's path-insensitive s_waitcnt insertion lets one role's pending loads tax another's: round 5 found an
// s_waitcnt vmcnt(0) in k_att's LOADER loop -- draining its DMA queue -- that guarded a register a consumer-side load had been given.)
__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
__device__ __forceinline__ int block_lo(int n) { return (int)(((unsigned)blockIdx.x * (unsigned)n) / gridDim.x); }
__device__ __forceinline__ int block_hi(int n) { return (int)((((unsigned)blockIdx.x + 1u) * (unsigned)n) / gridDim.x); }
constexpr unsigned VOCAB = 50277u;
constexpr float QLIM = 4194000.0f;       // |quantised activation| <= QLIM < 2^22
constexpr double QOFF = 4194304.0;       // 2^22: limbs hold q + 2^22 as an unsigned 23-bit number
constexpr float QMAGIC = 12582912.0f;    // 1.5 * 2^23: float(q + QMAGIC) has q + 2^22 in its low three bytes

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

// per-token control block, lives in device memory so a captured hipGraph can be replayed for
// any token / state slot / logits row (and so the device-side argmax can feed the next step)
struct Ctl {
    unsigned long long token;
    unsigned int slot;     // state slot (PARRALEL mode: sequence index; GPT mode: 0)
    unsigned int out_row;  // logits row
    unsigned int step;     // greedy-decode step counter
    unsigned int pad;
};

// 64-lane reductions run on the DPP network (VALU-latency steps) instead of six dependent
// ds_bpermute round trips through the LDS crossbar per reduction: xor-1 / xor-2 inside quads,
// rotate by 4 and 8 inside each row of 16, then row_bcast:15 / row_bcast:31 fold the four rows into
// lane 63; readlane makes the result wave-uniform.  Lanes disabled by a row mask read 0 (`old`).
template <int CTRL, int ROW_MASK, bool BOUND>
__device__ __forceinline__ double dpp_f64(double v)
{
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)u, CTRL, ROW_MASK, 0xf, BOUND);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), CTRL, ROW_MASK, 0xf, BOUND);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double wave_sum(double v)
{
    v += dpp_f64<0xB1, 0xf, true>(v);
    v += dpp_f64<0x4E, 0xf, true>(v);
    v += dpp_f64<0x124, 0xf, true>(v);
    v += dpp_f64<0x128, 0xf, true>(v);
    v += dpp_f64<0x142, 0xa, false>(v);
    v += dpp_f64<0x143, 0xc, false>(v);
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, 63), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), 63);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
template <int CTRL, int ROW_MASK, bool BOUND>
__device__ __forceinline__ float dpp_f32(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, BOUND));
}
// max of NON-NEGATIVE values (disabled lanes contribute 0)
__device__ __forceinline__ float wave_max(float v)
{
    v = fmaxf(v, dpp_f32<0xB1, 0xf, true>(v));
    v = fmaxf(v, dpp_f32<0x4E, 0xf, true>(v));
    v = fmaxf(v, dpp_f32<0x124, 0xf, true>(v));
    v = fmaxf(v, dpp_f32<0x128, 0xf, true>(v));
    v = fmaxf(v, dpp_f32<0x142, 0xa, false>(v));
    v = fmaxf(v, dpp_f32<0x143, 0xc, false>(v));
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ unsigned wave_sum_dpp(unsigned v)
{
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true);    // quad_perm [1,0,3,2]
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, true);    // quad_perm [2,3,0,1]
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xf, 0xf, true);   // row_ror:4
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, true);   // row_ror:8
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1,3
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2,3
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// workgroup-wide sum of K doubles; every thread gets the totals.  `red` = NW*K doubles of LDS that no
// later reduction of the same kernel reuses before all waves have read them (callers hand out
// distinct regions of the 1 KiB scratch), so ONE barrier per reduction.
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double *red)
{
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = wave_sum(v[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) red[w * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < NW; i++) s += red[i * K + k];
        v[k] = s;
    }
}
// workgroup-wide max of K floats (same scratch discipline)
template <int K>
__device__ __forceinline__ void block_max(float (&v)[K], double *redd)
{
    float *red = reinterpret_cast<float *>(redd);
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = wave_max(v[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) red[w * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NW; i++) s = fmaxf(s, red[i * K + k]);
        v[k] = s;
    }
}
// scratch regions (in doubles) of the RED_BYTES block: NW*K <= 24 doubles each
constexpr int RED_STATS = 0, RED_MAX = 24, RED_OFFS = 48, RED_PART = 72;

// ------------------------------------------------------------------------------------------
// Staged activation vectors.  Element j of a vector belongs to the 16-element piece c = j/16,
// which lane c%64 consumes at step c/64 together with weight bytes [16c, 16c+16) of a row.
// LDS image per vector: [step][limb 0..2][lane][4 dwords]; dword q of a lane holds limb b of
// elements 16c+4q .. 16c+4q+3 (byte e = element 4q+e), i.e. exactly the operand v_dot4_u32_u8
// needs against dword q of the lane's 16 weight bytes.  A lane's ds_read_b128 of one limb plane is
// lane-consecutive (conflict-free).  S*768 dwords (3 KiB per step) per vector.
template <int S> __host__ __device__ __forceinline__ constexpr int xvd() { return S * 768; }

// quantise 4 consecutive elements (quad qd = j/4) with 1/scale `inv_s` and store their 3 limb dwords.
// real == false writes zero limbs: padding must contribute nothing to the integer sums (it is
// outside the row sums used for the 2^22 offset correction).
__device__ __forceinline__ void stage_quad(unsigned *xq, int qd, const float (&xr)[4], float inv_s, bool real)
{
    // One fma per element does scale, round-to-nearest-even and offset: for |x * inv_s| < 2^22 the
    // float x * inv_s + 1.5 * 2^23 has ulp 1 and bit pattern 0x4B400000 + q, i.e. its bytes 0..2 are the
    // three limbs of q + 2^22.  v_perm_b32 then transposes 4 elements x 3 bytes into 3 limb dwords.
    unsigned t[4];
#pragma unroll
    for (int e = 0; e < 4; e++) t[e] = __float_as_uint(fmaf(xr[e], inv_s, QMAGIC));
    const unsigned p01 = __builtin_amdgcn_perm(t[1], t[0], 0x05010400u);   // {t0.b0, t1.b0, t0.b1, t1.b1}
    const unsigned p23 = __builtin_amdgcn_perm(t[3], t[2], 0x05010400u);
    const unsigned h01 = __builtin_amdgcn_perm(t[1], t[0], 0x0c0c0602u);   // {t0.b2, t1.b2, 0, 0}
    const unsigned h23 = __builtin_amdgcn_perm(t[3], t[2], 0x0c0c0602u);
    const unsigned d0 = __builtin_amdgcn_perm(p23, p01, 0x05040100u);
    const unsigned d1 = __builtin_amdgcn_perm(p23, p01, 0x07060302u);
    const unsigned d2 = __builtin_amdgcn_perm(h23, h01, 0x05040100u);
    const int c = qd >> 2, q = qd & 3;
    unsigned *p = xq + ((((c >> 6) * 3) * 64 + (c & 63)) << 2) + q;
    p[0] = real ? d0 : 0u;
    p[256] = real ? d1 : 0u;
    p[512] = real ? d2 : 0u;
}
__device__ __forceinline__ float inv_scale(float amax) { return QLIM / fmaxf(amax, 1e-30f); }
__device__ __forceinline__ double scale_of(float amax) { return (double)fmaxf(amax, 1e-30f) / (double)QLIM; }
// integer sums of one row -> real value of sum_j u_j * x_j
__device__ __forceinline__ float row_value(unsigned long long T, unsigned rowsum, double scale)
{
    return (float)(scale * ((double)(long long)T - QOFF * (double)rowsum));
}

// which staged vector row r of a group multiplies with
enum { PAT_SHARED = 0,   // all rows use vector 0              (att_out, head, mm8)
       PAT_PER_ROW = 1,  // row r uses vector r                (K/V/R; the 4 quarter-rows of ffn_v)
       PAT_FFN_RK = 2 }; // rows 0..3 vector 0, row 4 vector 1 (4 ffn_k rows + 1 ffn_r row)
template <int PAT> __device__ __forceinline__ constexpr int xsel(int r)
{
    return PAT == PAT_SHARED ? 0 : (PAT == PAT_PER_ROW ? r : (r < 4 ? 0 : 1));
}
template <int PAT, int R> __device__ __forceinline__ constexpr int nvec()
{
    return PAT == PAT_SHARED ? 1 : (PAT == PAT_PER_ROW ? R : 2);
}

// ------------------------------------------------------------------------------------------
// Row-group streaming.  A group = R rows `stride` bytes apart, each `chunks` 16-byte pieces long;
// piece c belongs to lane c%64 at step c/64, so one step of one row is a 1 KiB coalesced
// non-temporal wave load.  Lanes past the end of a row (rows that are not a multiple of 1 KiB)
// re-read the row's last piece instead of branching: the staged limbs are zero there, and a
// predicated load would make hipcc drain vmcnt(0) at the branch join.
template <int R, int S>
__device__ __forceinline__ void step_load(u32x4 (&w)[R][S], int s, const uint8_t *__restrict__ base,
                                          size_t stride, int chunks, int lane, unsigned mask = 0xffffffffu)
{
    // address = wave-uniform row pointer (SGPR pair) + 32-bit per-lane byte offset (one VGPR per
    // step): global_load_dwordx4 v, v_off, s[base] -- no 64-bit per-(row,step) address registers.
    // mask == 0 turns the step into R loads of one 16-byte piece (see group_dot's refill).
    int c = lane + 64 * s;
    c = c < chunks ? c : chunks - 1;
    const unsigned off = ((unsigned)c << 4) & mask;
#pragma unroll
    for (int r = 0; r < R; r++)
        w[r][s] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(base + r * stride + off));
}
// steps [S0, S1) of a group, in consumption order (step-major)
template <int R, int S, int S0, int S1>
__device__ __forceinline__ void group_load(u32x4 (&w)[R][S], const uint8_t *__restrict__ base,
                                           size_t stride, int chunks, int lane)
{
#pragma unroll
    for (int s = S0; s < S1; s++) step_load<R, S>(w, s, base, stride, chunks, lane);
}
// How many steps of the first group are requested BEFORE the prologue runs.  A wave that asks for
// more than the memory pipe accepts stalls at issue (in-order) and its prologue waits with it; a
// wave that asks for too little leaves HBM idle while the prologue computes.  Tuned on MI355X.
#ifndef RWKV_PRE_STEPS
#define RWKV_PRE_STEPS 2
#endif
template <int S> __device__ __forceinline__ constexpr int pre_steps() { return RWKV_PRE_STEPS < S ? RWKV_PRE_STEPS : S; }

// Integer dot products of the loaded group with the staged vector(s): T[r] = sum_j u_rj * q'_j
// (q' = 23-bit unsigned limb value), every lane gets all R sums.
//  * The LDS reads of the limb pieces are software-pipelined one (step, vector) item ahead and
//    pinned with sched barriers, so at most two 12-dword pieces are live.
//  * Refill: as soon as step s of this group has been consumed its registers are re-loaded with
//    step s of the NEXT group (`next`), so the wave keeps R*S loads in flight across groups
//    instead of draining and restarting the memory pipe at every group boundary.  The refill is
//    unconditional and branch-free (a branch would make hipcc's waitcnt pass merge the two paths
//    and wait for the refill itself; two template copies in sibling branches get their common
//    code hoisted and spilled): after a wave's LAST group, `next_valid` = false degrades the refill
//    to R*S loads of one and the same 16-byte piece (one L1-resident line), which nobody waits for.
template <int R, int S, int PAT>
__device__ __forceinline__ void group_dot(u32x4 (&w)[R][S], const unsigned *xq, int lane, unsigned long long (&T)[R],
                                          const uint8_t *__restrict__ next, size_t stride, int chunks, bool next_valid)
{
    constexpr int NV = nvec<PAT, R>();
    constexpr int NI = S * NV;
    constexpr int XVD = xvd<S>();
    const unsigned mask = next_valid ? 0xffffffffu : 0u;
    const size_t nstride = next_valid ? stride : 0;
    unsigned acc[R][3];
#pragma unroll
    for (int r = 0; r < R; r++) { acc[r][0] = acc[r][1] = acc[r][2] = 0u; }
    u32x4 x[2][3];
    const u32x4 *xb = reinterpret_cast<const u32x4 *>(xq) + lane;
#pragma unroll
    for (int b = 0; b < 3; b++) x[0][b] = xb[b * 64];
#pragma unroll
    for (int it = 0; it < NI; it++) {
        const int s = it / NV, v = it % NV;
        if (it + 1 < NI) {
            const int s1 = (it + 1) / NV, v1 = (it + 1) % NV;
            const u32x4 *p = xb + (v1 * (XVD >> 2)) + (s1 * 3) * 64;
#pragma unroll
            for (int b = 0; b < 3; b++) x[(it + 1) & 1][b] = p[b * 64];
        }
#pragma unroll
        for (int r = 0; r < R; r++)
            if (xsel<PAT>(r) == v) {
#pragma unroll
                for (int b = 0; b < 3; b++)
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        acc[r][b] = __builtin_amdgcn_udot4(w[r][s][q], x[it & 1][b][q], acc[r][b], false);
                // pin the partial sums here so the dot products stay between their LDS reads
                asm volatile("" : "+v"(acc[r][0]), "+v"(acc[r][1]), "+v"(acc[r][2]));
            }
        __builtin_amdgcn_sched_barrier(0);
        if (v == NV - 1) {
            step_load<R, S>(w, s, next, nstride, chunks, lane, mask);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // each limb total fits 32 bits (N * 255 * 255 < 2^32 for N <= 66051), so the three planes are
    // reduced as u32 and combined afterwards on wave-uniform values
#pragma unroll
    for (int r = 0; r < R; r++) {
        const unsigned t0 = wave_sum_dpp(acc[r][0]), t1 = wave_sum_dpp(acc[r][1]), t2 = wave_sum_dpp(acc[r][2]);
        T[r] = (unsigned long long)t0 + ((unsigned long long)t1 << 8) + ((unsigned long long)t2 << 16);
    }
}

// ------------------------------------------------------------------------------------------
// LayerNorm "sites": where a LayerNorm + token-shift mix feeds a GEMV (ln1 -> K/V/R, ln2 -> ffn k/r,
// ln_out -> head).  Every consumer workgroup needs the whole mixed vector, and computing it per
// workgroup from scratch (x, state, ~10 parameter vectors, two dependent reductions) was the largest
// loss of the first design (phase timeline: ~6 us before the first dot of a 22 us kernel).  So the
// work is split by OWNERSHIP.  With xhat = (x - mean) * rstd the staged vector of a site is
//     v_m[j] = r_m (mix_m (lnw xhat + lnb) + (1 - mix_m) prev) = C_m[j] * xhat[j] + B_m[j]
//     C_m = r_m mix_m lnw                          (static, packed at load)
//     B_m = r_m (mix_m lnb + (1 - mix_m) prev[j])  (needs only the OLD state: emitted by the row owner)
// and the offset scalar  S_m = sum_j o_m f_m[j] = rstd * PA_m - mean rstd * TC_m + PB_m  with
// PA_m = sum Co_m x,  PB_m = sum (BoL_m + BoP_m prev),  TC_m = sum Co_m  (Co = o mix lnw, ...).
// The kernel whose lanes OWN rows of x (k_first / k_attout / k_ffnv) emits B_m[j] for its rows and one
// partial tuple per workgroup {sum x, sum x^2, PA_m, PB_m; max|x|, max|B_m|}; the consumer reduces
// the tuples in ONE round (mean, rstd, S_m, and an upper bound of max|v_m| for the fixed-point scale:
// maxC_m (max|x| + |mean|) rstd + max|B_m|), then only does C*xhat + B per element.  The new state
// (ln output of this token) is committed by the row owner that overwrites x, from (mean, rstd)
// published by the consumer.  Prologue traffic drops from 48-64 to 24-32 bytes per channel.
// optional phase timeline (debug / tuning): lane 0 of every wave stamps the 100 MHz wall clock
// into tl[((block * NW) + wave) * 8 + phase].  tl == nullptr in production.
__device__ __forceinline__ void tl_stamp(unsigned long long *tl, int phase)
{
    if (tl) {
        __builtin_amdgcn_sched_barrier(0);
        const unsigned long long t = wall_clock64();
        if ((threadIdx.x & 63) == 0) tl[((size_t)blockIdx.x * NW + (threadIdx.x >> 6)) * 8 + phase] = t;
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <int NV> __host__ __device__ constexpr int site_pw() { return NV == 3 ? 16 : NV == 2 ? 12 : 8; }
struct SiteStatic {               // one site of one layer
    const float *C;               // [NV][D]  consumer side
    const float *P;               // [D][PW]  producer side: per channel, per vector m: BL, BP, Co, BoL, BoP at [m*5 + k]
    const double *TC;             // [NV]
    const float *maxC;            // [NV]
    double invD, invDm1;          // 1/D, 1/(D-1)
};
struct SiteDyn {
    float *B;                     // [NV][D]
    double *pd;                   // [n_part][8]: sum x, sum x^2, PA_0..2, PB_0..2
    float *pf;                    // [n_part][4]: max|x|, max|B_0..2|
    double *lnstat;               // [2]: mean, rstd of this site (written by consumer workgroup 0)
    int n_part;
};
template <int NV> struct SiteAcc {
    double d[8];
    float f[4];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int k = 0; k < 8; k++) d[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) f[k] = 0.f;
    }
};
template <int NV> struct SitePre { f32x4 p[site_pw<NV>() / 4]; };
// row owner, before its dot product: request the producer-side constants of channel j
template <int NV>
__device__ __forceinline__ void site_prefetch(const SiteStatic &st, int j, SitePre<NV> &pre)
{
    constexpr int PW = site_pw<NV>();
#pragma unroll
    for (int k = 0; k < PW / 4; k++) pre.p[k] = reinterpret_cast<const f32x4 *>(st.P + (size_t)j * PW)[k];
}
// row owner: emit B_m[j] and accumulate this thread's share of the workgroup tuple
template <int NV>
__device__ __forceinline__ void site_emit(const SitePre<NV> &pre, const SiteDyn &dy, int D, int j, double x, double prev, SiteAcc<NV> &acc)
{
    acc.d[0] += x;
    acc.d[1] += x * x;
    acc.f[0] = fmaxf(acc.f[0], (float)fabs(x) * 1.0000002f);   // round-up guard: used as an upper bound
#pragma unroll
    for (int m = 0; m < NV; m++) {
        const float bl = pre.p[(m * 5 + 0) >> 2][(m * 5 + 0) & 3], bp = pre.p[(m * 5 + 1) >> 2][(m * 5 + 1) & 3];
        const float co = pre.p[(m * 5 + 2) >> 2][(m * 5 + 2) & 3];
        const float bol = pre.p[(m * 5 + 3) >> 2][(m * 5 + 3) & 3], bop = pre.p[(m * 5 + 4) >> 2][(m * 5 + 4) & 3];
        const float b = (float)((double)bl + (double)bp * prev);
        dy.B[(size_t)m * D + j] = b;
        acc.d[2 + m] += (double)co * x;
        acc.d[5 + m] += (double)bol + (double)bop * prev;
        acc.f[1 + m] = fmaxf(acc.f[1 + m], fabsf(b));
    }
}
// all threads: fold the accumulators into this workgroup's tuple.  LIVE = lanes per wave that hold
// one (the row owners are lanes 0..R-1 of every wave; 64 = every lane).  scratch: NW*LIVE*12 words of
// LDS (or the 640-byte reduction block for LIVE == 64) that no wave still reads.
template <int NV, int LIVE>
__device__ __forceinline__ void site_publish(SiteAcc<NV> &acc, const SiteDyn &dy, void *scratch)
{
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    constexpr int NE = LIVE == 64 ? NW : NW * LIVE;   // entries to add up
    double *red = reinterpret_cast<double *>(scratch);
    float *redf = reinterpret_cast<float *>(red + NE * 8);
    if (LIVE == 64) {
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (k < 2 || (k - 2) % 3 < NV) acc.d[k] = wave_sum(acc.d[k]);
#pragma unroll
        for (int k = 0; k < 1 + NV; k++) acc.f[k] = wave_max(acc.f[k]);
    }
    if (lane < (LIVE == 64 ? 1 : LIVE)) {
        const int e = LIVE == 64 ? w : w * LIVE + lane;
#pragma unroll
        for (int k = 0; k < 8; k++) red[e * 8 + k] = acc.d[k];
#pragma unroll
        for (int k = 0; k < 4; k++) redf[e * 4 + k] = acc.f[k];
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        double t = 0.0;
        for (int i = 0; i < NE; i++) t += red[i * 8 + threadIdx.x];
        dy.pd[(size_t)blockIdx.x * 8 + threadIdx.x] = t;
    } else if (threadIdx.x < 12) {
        float t = 0.f;
        for (int i = 0; i < NE; i++) t = fmaxf(t, redf[i * 4 + (threadIdx.x - 8)]);
        dy.pf[(size_t)blockIdx.x * 4 + (threadIdx.x - 8)] = t;
    }
}
template <int NV> struct SiteRed {
    double mean, rstd;
    double S[NV];
    float amax[NV];
};
// consumer, step 1 (first loads of the kernel): this thread's partial tuple
struct SiteTuple { f64x2 d[4]; f32x4 f; };
__device__ __forceinline__ void site_tuple_load(const SiteDyn &dy, SiteTuple &t)
{
    const int i = (int)threadIdx.x < dy.n_part ? threadIdx.x : 0;
#pragma unroll
    for (int k = 0; k < 4; k++) t.d[k] = reinterpret_cast<const f64x2 *>(dy.pd)[i * 4 + k];
    t.f = reinterpret_cast<const f32x4 *>(dy.pf)[i];
}
// consumer, step 2: one reduction round -> LayerNorm statistics, offset scalars, scale bounds
// NWR = number of waves taking part (waves 0..NWR-1).  spin != nullptr: the waves meet on an LDS
// counter (zeroed by the caller behind an earlier barrier) instead of the workgroup barrier, so the
// remaining waves of the workgroup need not take part.
template <int NV, int NWR = NW>
__device__ __forceinline__ void site_reduce(const SiteStatic &st, const SiteDyn &dy, const SiteTuple &t, int D, double *red, SiteRed<NV> &out,
                                            const double (&tc)[NV], const float (&mc)[NV], unsigned long long *tl = nullptr, unsigned *spin = nullptr)
{
    float *redf = reinterpret_cast<float *>(red + NW * 8);
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool real = (int)threadIdx.x < dy.n_part;
    double d[8];
    float f[4];
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = real ? t.d[k >> 1][k & 1] : 0.0;
#pragma unroll
    for (int k = 0; k < 4; k++) f[k] = real ? t.f[k] : 0.f;
#pragma unroll
    for (int k = 0; k < 8; k++)
        if (k < 2 || (k - 2) % 3 < NV) d[k] = wave_sum(d[k]);
#pragma unroll
    for (int k = 0; k < 1 + NV; k++) f[k] = wave_max(f[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 8; k++) red[w * 8 + k] = d[k];
#pragma unroll
        for (int k = 0; k < 4; k++) redf[w * 4 + k] = f[k];
    }
    tl_stamp(tl, 3);
    if (spin) {
        if (lane == 0) __hip_atomic_fetch_add(spin, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        while (__hip_atomic_load(spin, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < (unsigned)NWR) __builtin_amdgcn_s_sleep(1);
    } else {
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
        if (k < 2 || (k - 2) % 3 < NV) {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < NWR; i++) s += red[i * 8 + k];
            d[k] = s;
        }
    }
#pragma unroll
    for (int k = 0; k < 1 + NV; k++) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NWR; i++) s = fmaxf(s, redf[i * 4 + k]);
        f[k] = s;
    }
    out.mean = d[0] * st.invD;
    const double var = (d[1] - d[0] * out.mean) * st.invDm1;   // reference: (D-1), no epsilon (rwkv.cu:43-44,53)
    out.rstd = rsqrt(var);
    const double mrs = out.mean * out.rstd;
#pragma unroll
    for (int m = 0; m < NV; m++) {
        out.S[m] = out.rstd * d[2 + m] - mrs * tc[m] + d[5 + m];
        out.amax[m] = (mc[m] * (float)(((double)f[0] + fabs(out.mean)) * out.rstd) + f[1 + m]) * 1.0001f;
    }
}
__device__ __forceinline__ void load_quad_f64(const double *p, int qd, double (&out)[4])
{
    const f64x2 a = reinterpret_cast<const f64x2 *>(p)[qd * 2], b = reinterpret_cast<const f64x2 *>(p)[qd * 2 + 1];
    out[0] = a[0]; out[1] = a[1]; out[2] = b[0]; out[3] = b[1];
}
// consumer, step 3: v_m = C_m * xhat + B_m for this thread's quads, quantised and staged
template <int NV, int NQ, int S, int NTP = NT>
__device__ __forceinline__ void site_stage(const double (&xl)[NQ][4], const f32x4 (&Cq)[NQ][NV], const f32x4 (&Bq)[NQ][NV],
                                           const SiteRed<NV> &sr, unsigned *xq, int nqd)
{
    constexpr int XVD = xvd<S>();
    const float rstdf = (float)sr.rstd;
#pragma unroll
    for (int i = 0; i < NQ; i++) {
        const int qd = threadIdx.x + i * NTP;
        if (qd < S * 256) {
            float xh[4];   // the subtraction stays in f64 (|mean| may dwarf the deviation); the rest is f32
#pragma unroll
            for (int e = 0; e < 4; e++) xh[e] = (float)(xl[i][e] - sr.mean) * rstdf;
#pragma unroll
            for (int m = 0; m < NV; m++) {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; e++) v[e] = fmaf(Cq[i][m][e], xh[e], Bq[i][m][e]);
                stage_quad(xq + m * XVD, qd, v, inv_scale(sr.amax[m]), qd < nqd);
            }
        }
    }
}
// ------------------------------------------------------------------------------------------
// Kernel prologues.  What the first microseconds of a kernel look like decides a third of its run
// time, and three measured properties of the CU's vector-memory path shape them:
//  * data returns IN ORDER per CU (no hit-under-miss): a prologue load queued behind weight loads
//    arrives after them, however warm its line is in L2;
//  * the path holds only ~16 KB of requests: a wave that asks for more blocks at issue until HBM has
//    delivered -- and a blocked wave cannot run the prologue or reach a barrier;
//  * every workgroup reads the same ~100 KB of prologue inputs, 3.6 MB per XCD through one L2.
// SPLIT prologues therefore give the waves roles until the vector is staged: waves 0..NW/2-1 request
// the prologue inputs of the WHOLE vector, an order barrier lets those requests enter the pipe first,
// then waves NW/2.. ("loaders") request their entire first row group -- they block at issue, which
// is the point: the weight stream starts in the second microsecond and runs under the prologue --
// while the prologue waves reduce (meeting on an LDS counter, not the workgroup barrier), quantise
// and stage, publish the scalars through LDS, and join the loaders at the "staged" barrier.
// which kernels use the role split (bit 0 k_att, 1 k_attout, 2 k_ffn_rk, 3 k_ffnv, 4 k_head): measured per kernel
#ifndef RWKV_SPLIT
#define RWKV_SPLIT 23
#endif
// The small overlay at double RED_BC of the reduction scratch, as 32-bit words: [0..7] the scalars the prologue waves publish (offsets [0..3],
// amax [4..7] per vector), [8] the word the prologue waves meet on, [9] the row-group counter (below).  Every reader goes through these three.
constexpr int RED_BC = 96;
static_assert(RED_BC * 8 + 10 * 4 <= RED_BYTES, "the overlay lies inside the reduction scratch");
__device__ __forceinline__ float *red_bc(double *red) { return reinterpret_cast<float *>(red + RED_BC); }
__device__ __forceinline__ unsigned *red_spin(double *red) { return reinterpret_cast<unsigned *>(red + RED_BC) + 8; }

// Row groups of a workgroup are handed out through an LDS counter (DYN): the waves that ran the
// prologue start their first group late, the others take more of the remaining groups.  The counter
// lives next to the published scalars and is set by thread 0 before the prologue's barriers.
#ifndef RWKV_HEAD_R
#define RWKV_HEAD_R 2      // rows per group in k_head (measured: 2 -> 35.8, 3 -> 36.2, 4 -> 36.8, 5 -> 38.0 us at 7B)
#endif
__device__ __forceinline__ unsigned *group_counter(double *red) { return reinterpret_cast<unsigned *>(red + RED_BC) + 9; }
__device__ __forceinline__ int next_group(unsigned *ctr)
{
    unsigned v = 0;
    if ((threadIdx.x & 63) == 0) v = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return __builtin_amdgcn_readfirstlane((int)v);
}

// The streaming loop of every decode kernel.  A wave owns the groups it draws from the workgroup's LDS counter; group
// indices drawn later are larger, so the OLDEST outstanding group is tested and a miss ends the loop.  Per group:
// pre(g) requests the epilogue's inputs (before the dot issues the refills: a load placed after them would, by in-order
// vmcnt, wait for the whole next group to land), group_dot consumes the group's registers and refills them step by step
// with the group drawn now, epi(g, T, in) finishes the rows.  base(g) = weight address of a valid group.
// One buffer of weight registers per wave: the CU's memory pipe accepts only ~16 KB of requests, and a second buffer kept a loader
// wave blocked at issue twice as long -- 8 % slower at 7B (485 vs 528 tokens/s, profiles/r02/decode_variants_nbuf.txt).
template <int R, int S, int PAT, class Base, class Pre, class Epi>
__device__ __forceinline__ void stream_groups(u32x4 (&wA)[R][S], int gA, int g0, int g1, unsigned *gctr,
                                              const unsigned *xq, int lane, size_t stride, int chunks, Base base, Pre pre, Epi epi)
{
    while (gA < g1) {
        const int gn = next_group(gctr);
        const bool nv = gn < g1;
        const auto in = pre(gA);
        unsigned long long T[R];
        group_dot<R, S, PAT>(wA, xq, lane, T, base(nv ? gn : g0), stride, chunks, nv);
        epi(gA, T, in);
        gA = gn;
    }
}
// first group of a wave (g0 + wave) and the counter's start; set by thread 0 before the prologue's barriers
__device__ __forceinline__ void first_groups(int g0, int wave, unsigned *gctr, int &gA)
{
    gA = g0 + wave;
    if (threadIdx.x == 0) *gctr = (unsigned)(g0 + NW);
}
// workgroup-wide sum of one double and max of one non-negative float in ONE barrier (the kernels' closing reduction)
__device__ __forceinline__ void block_sum_max(double &sv, float &mv, double *red)
{
    float *redf = reinterpret_cast<float *>(red + NW);
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    sv = wave_sum(sv);
    mv = wave_max(mv);
    if (lane == 0) { red[w] = sv; redf[w] = mv; }
    __syncthreads();
    double s = 0.0; float m = 0.f;
#pragma unroll
    for (int i = 0; i < NW; i++) { s += red[i]; m = fmaxf(m, redf[i]); }
    sv = s; mv = m;
}

// LayerNorm-site consumer (k_att, k_ffn_rk, k_head): on return the NV vectors are staged in xq,
// sr.S / sr.amax are valid in every wave and w holds (requests for) the wave's first row group.
template <int NV, int R, int S, bool SPLIT>
__device__ __forceinline__ void site_open(const SiteStatic &st, const SiteDyn &dy, const double *x, int D, double *red, unsigned *xq,
                                          u32x4 (&w)[R][S], const uint8_t *wb, size_t stride,
                                          SiteRed<NV> &sr, bool publish_stats, unsigned long long *tl)
{
    const int lane = threadIdx.x & 63, wave = wave_id();
    const int chunks = D >> 4, nqd = D >> 2;
    constexpr int NTP = SPLIT ? NT / 2 : NT, NWP = NTP / 64, NQP = (S * 256 + NTP - 1) / NTP;
    float *bc = red_bc(red);
    unsigned *spin = red_spin(red);
    if (SPLIT && wave >= NWP) {
        __syncthreads();   // order: the prologue waves' requests are in the memory pipe
        group_load<R, S, 0, S>(w, wb, stride, chunks, lane);
        tl_stamp(tl, 2);
        __syncthreads();   // staged
    } else {
        // the site's static scalars are read here, not where they are used: behind the reduction's barrier the
        // compiler may not hoist them, and a cold scalar load there sits on the prologue's critical path
        double tc[NV];
        float mc[NV];
#pragma unroll
        for (int m = 0; m < NV; m++) { tc[m] = st.TC[m]; mc[m] = st.maxC[m]; }
        SiteTuple tup;
        site_tuple_load(dy, tup);
        double xl[NQP][4];
        f32x4 Cq[NQP][NV], Bq[NQP][NV];
#pragma unroll
        for (int i = 0; i < NQP; i++) {
            const int qd = threadIdx.x + i * NTP, qc = qd < nqd ? qd : nqd - 1;
            load_quad_f64(x, qc, xl[i]);
#pragma unroll
            for (int m = 0; m < NV; m++) {
                Cq[i][m] = reinterpret_cast<const f32x4 *>(st.C + (size_t)m * D)[qc];
                Bq[i][m] = reinterpret_cast<const f32x4 *>(dy.B + (size_t)m * D)[qc];
            }
        }
        tl_stamp(tl, 1);
        if (SPLIT) {
            if (threadIdx.x == 0) *spin = 0u;
            __syncthreads();   // order (see the loader role)
            site_reduce<NV, NWP>(st, dy, tup, D, red, sr, tc, mc, tl, spin);
        } else {
            // a small pre-issue of the weight stream; more would block this wave's prologue
            group_load<R, S, 0, pre_steps<S>()>(w, wb, stride, chunks, lane);
            tl_stamp(tl, 2);
            site_reduce<NV, NWP>(st, dy, tup, D, red, sr, tc, mc, tl);
        }
        if (publish_stats && blockIdx.x == 0 && threadIdx.x == 0) { dy.lnstat[0] = sr.mean; dy.lnstat[1] = sr.rstd; }
        tl_stamp(tl, 4);
        site_stage<NV, NQP, S, NTP>(xl, Cq, Bq, sr, xq, nqd);
        if (SPLIT && threadIdx.x == 0) {
#pragma unroll
            for (int m = 0; m < NV; m++) { bc[m] = (float)sr.S[m]; bc[4 + m] = sr.amax[m]; }
        }
        __syncthreads();   // staged
        group_load<R, S, SPLIT ? 0 : pre_steps<S>(), S>(w, wb, stride, chunks, lane);
    }
    if (SPLIT) {
#pragma unroll
        for (int m = 0; m < NV; m++) { sr.S[m] = (double)bc[m]; sr.amax[m] = bc[4 + m]; }
    }
    tl_stamp(tl, 5);
}

// Plain-vector consumer (k_attout: NVEC = 1; k_ffnv: the four quarter vectors of the hidden vector).
// The producer left the pre-scaled vector and per-workgroup partials of the offset sum and of max|.|.
template <int NVEC, int R, int S, bool SPLIT>
__device__ __forceinline__ void vec_open(const float *vec, const double *partS, const float *partM, int n_part, int D, double *red,
                                         unsigned *xq, u32x4 (&w)[R][S], const uint8_t *wb, size_t stride,
                                         float &Sf, float &amax, unsigned long long *tl)
{
    constexpr int XVD = xvd<S>();
    const int lane = threadIdx.x & 63, wave = wave_id();
    const int chunks = D >> 4, nqd = D >> 2;
    constexpr int NTP = SPLIT ? NT / 2 : NT, NWP = NTP / 64, NQP = (S * 256 + NTP - 1) / NTP;
    float *bc = red_bc(red);
    unsigned *spin = red_spin(red);
    if (SPLIT && wave >= NWP) {
        __syncthreads();   // order
        group_load<R, S, 0, S>(w, wb, stride, chunks, lane);
        tl_stamp(tl, 2);
        __syncthreads();   // staged
    } else {
        double ps = partS[(int)threadIdx.x < n_part ? threadIdx.x : 0];
        float pm = partM[(int)threadIdx.x < n_part ? threadIdx.x : 0];
        float vl[NVEC][NQP][4];
#pragma unroll
        for (int q = 0; q < NVEC; q++)
#pragma unroll
            for (int i = 0; i < NQP; i++) {
                const int qd = threadIdx.x + i * NTP, qc = qd < nqd ? qd : nqd - 1;
                const f32x4 t = reinterpret_cast<const f32x4 *>(vec + (size_t)q * D)[qc];
                vl[q][i][0] = t[0]; vl[q][i][1] = t[1]; vl[q][i][2] = t[2]; vl[q][i][3] = t[3];
            }
        tl_stamp(tl, 1);
        if (SPLIT) {
            if (threadIdx.x == 0) *spin = 0u;
            __syncthreads();   // order
        } else {
            group_load<R, S, 0, pre_steps<S>()>(w, wb, stride, chunks, lane);
            tl_stamp(tl, 2);
        }
        if ((int)threadIdx.x >= n_part) { ps = 0.0; pm = 0.f; }
        {   // scale and offset from the producer's per-workgroup partials: one reduction round
            float *redf = reinterpret_cast<float *>(red + RED_MAX);
            const double ws = wave_sum(ps);
            const float wm = wave_max(pm);
            if (lane == 0) { red[RED_OFFS + wave] = ws; redf[wave] = wm; }
            tl_stamp(tl, 3);
            if (SPLIT) {
                if (lane == 0) __hip_atomic_fetch_add(spin, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                while (__hip_atomic_load(spin, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < (unsigned)NWP) __builtin_amdgcn_s_sleep(1);
            } else {
                __syncthreads();
            }
            double ts = 0.0; float tm = 0.f;
#pragma unroll
            for (int i = 0; i < NWP; i++) { ts += red[RED_OFFS + i]; tm = fmaxf(tm, redf[i]); }
            Sf = (float)ts; amax = tm;
        }
        tl_stamp(tl, 4);
#pragma unroll
        for (int q = 0; q < NVEC; q++)
#pragma unroll
            for (int i = 0; i < NQP; i++) {
                const int qd = threadIdx.x + i * NTP;
                if (qd < S * 256) stage_quad(xq + q * XVD, qd, vl[q][i], inv_scale(amax), qd < nqd);
            }
        if (SPLIT && threadIdx.x == 0) { bc[0] = Sf; bc[4] = amax; }
        __syncthreads();   // staged
        group_load<R, S, SPLIT ? 0 : pre_steps<S>(), S>(w, wb, stride, chunks, lane);
    }
    if (SPLIT) { Sf = bc[0]; amax = bc[4]; }
    tl_stamp(tl, 5);
}

// The dynamic LDS of a row-form decode kernel as byte offsets, regions in address order with nothing between them, by class (engine.hip's
// numbering: 1 k_att, 2 k_attout, 3 k_ffn_rk, 4 k_ffnv, 5 k_head): the reduction scratch, the staged vectors (k, v, r | the gated wkv | ffn k,
// ffn r | the four quarters of the hidden vector | ln_out), and k_head's argmax pair per wave.  The kernel takes its pointers from here,
// engine.hip the launch's bytes.  (The kernels add the offsets to the LDS array itself, smem + L.xq: through a helper that takes smem as a
// pointer the same constants compiled to other address arithmetic in 27 of the 30 instances, profiles/decode_host/isa_compare.txt.)
constexpr size_t CU_LDS_BYTES = 160 * 1024;
__host__ __device__ constexpr int row_nvec(int cls) { return cls == 1 ? 3 : cls == 3 ? 2 : cls == 4 ? 4 : 1; }
struct RowLds { size_t red = 0, xq = 0, bval = 0, bidx = 0, bytes = 0; };
__host__ __device__ constexpr RowLds row_lds_of(int cls, int S)
{
    RowLds l;
    l.xq = l.red + RED_BYTES;
    l.bval = l.xq + (size_t)row_nvec(cls) * S * xvd<1>() * 4;    // one staged vector = xvd<S>() words: 3 limb planes of S x 1 KiB
    l.bidx = l.bval + (cls == 5 ? NW * sizeof(float) : 0);
    l.bytes = l.bidx + (cls == 5 ? NW * sizeof(unsigned) : 0);
    return l;
}
// a kernel instance's description; asserts what the code relies on: u32x4 reads of the staged vectors, and that the widest model fits a CU
template <int CLS, int S> struct RowGeo {
    static constexpr RowLds L = row_lds_of(CLS, S);
    static_assert(L.xq % 16 == 0 && L.bval == L.xq + (size_t)row_nvec(CLS) * xvd<S>() * 4, "the staged vectors: 16-byte pieces, xvd<S>() words each");
    static_assert(row_lds_of(CLS, 5).bytes <= CU_LDS_BYTES, "LDS layout at S = 5");
};

// ------------------------------------------------------------------------------------------
// LDS-DMA primitives (the tile-form loaders, tile.hip.h, and the chunk path's staging, seq.hip.h).
// Loads into registers top out at ~10 B/clk per CU on this chip whatever is kept in flight;
// global_load_lds_dwordx4 -- the CU's DMA path from memory into LDS -- does not return through the vector register file.
// A loader wave issues the DMA of one unit (S KiB) as ONE asm statement (dma_unit_s, tile.hip.h), READS its vmcnt instead of waiting on it, keeps up to
// RWKV_RING_DEPTH pieces in flight and issues its first units in front of the workgroup's order barrier (RWKV_RING_PRE; per class in
// tile.hip.h); its consumers meet it on LDS counters only, and every wait loop is bounded (GLDS_SPIN) and reported through the
// context's error word (ring_report).
// The DMA is inline asm (hipcc would otherwise count it in vmcnt and drain it before every LDS access of the loader);
// m0 carries the wave-uniform LDS destination and is restored for the compiler.
__device__ __forceinline__ unsigned lds_addr(const void *p)
{
    return (unsigned)(unsigned long long)(const __attribute__((address_space(3))) void *)p;
}
// the same for data that OTHER workgroups of the XCD read as well (the chunk path's activation image): no "nt", it should stay in L2
__device__ __forceinline__ void dma_piece_shared(const uint8_t *src, unsigned lds_dst)
{
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(src), "s"(lds_dst) : "memory");
}
// First statement of every loader wave.  hipcc does not see the loader's DMA (inline asm), but it does remember every vector memory
// operation the wave issued BEFORE the role branch -- the debug timeline's store, a kernel-entry load -- and guards the registers those
// were given with s_waitcnt vmcnt(0) wherever the loader's code first reuses them: by the luck of register allocation that was inside
// the loader's loop in one round-5 build of k_att (12.3 -> 16.8 us: a drain of the DMA queue per group).  A wait the compiler DOES see
// (the builtin, not asm), placed where nothing of the DMA is in flight yet, settles its books: nothing is pending behind it.
__device__ __forceinline__ void loader_clean_slate() { __builtin_amdgcn_s_waitcnt(0x0F70); }      // vmcnt(0) expcnt(7) lgkmcnt(15)
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
constexpr int GLDS_SPIN = 1 << 18;    // bound of every wait loop (a lost hand-off must end the kernel, not hang the GPU)
// A wait that ran into its bound is RECORDED in a wave-uniform REGISTER (`fail`: no memory operation on any path that rejoins the
// streaming loops -- an error word stored from inside them, global or LDS, cost 3.5 % of the decode rate: hipcc's waitcnt insertion
// is path-insensitive, and the loader wave's instruction count is the stream's ceiling) and REPORTED once per wave, behind the
// kernel's closing barrier (ring_report), to the context's error word (mapped host memory; engine.hip device_check reads it after
// the stream synchronisation and fails the call with RWKV_E_DEVICE): the kernel still ends, but nobody is handed its results.
// codes: 1 loader found no room, 2 a unit never landed, 3 the prologue never staged (or the carried rows were never verified),
// 4 the loader's own DMA never completed.
__device__ __forceinline__ void wait_count(const unsigned *p, unsigned least, unsigned &fail)
{
    bool ok = false;
    for (int it = 0; it < GLDS_SPIN; it++) {
        if (__hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) >= least) { ok = true; break; }
        __builtin_amdgcn_s_sleep(1);
    }
    fail = ok ? fail : 3u;
}
__device__ __forceinline__ void ring_report(unsigned fail, unsigned *herr)
{
    if (fail != 0u && herr != nullptr && (threadIdx.x & 63) == 0) __hip_atomic_store(herr, fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// DMA pieces (1 KiB) the loader keeps in flight.  By Little's law the queueing delay of EVERY access of the CU is in-flight bytes /
// stream rate: 63 KiB at 23 KB/us = 2.7 us -- paid by the prologue's loads and, after the last issue, by the kernel's tail --
// while the stream itself is at full rate from ~24 KiB up (tools/dmabench.hip: depth 63 / 32 / 16 -> 7.3 / 7.3 / 6.0 TB/s).
// Round 6, with the matrix-core consumers (profiles/r06/depth_ab.txt): 24 .. 30 are a plateau 0.5 % above 32 at 7B, 20 falls off a cliff (-7.5 %);
// 28 with 20 in front of the barrier: 7B +0.55 %, 14B +0.8 %, 1B5 / 3B +0.1-0.2 %.
#ifndef RWKV_RING_DEPTH
#define RWKV_RING_DEPTH 28
#endif
// The weight stream starts BEFORE the workgroup's order barrier: the loader issues its first RWKV_RING_PRE units at once, thinly
// (RWKV_RING_PRE_DEPTH pieces in flight: the prologue's loads, issued ~1.4 us into the kernel, queue behind at most that), and
// only then joins the barrier that lets the prologue's requests into the pipe ahead of the deep stream.  The cold start of a
// kernel's stream (first translations, empty memory queues) then overlaps the prologue waves' own start-up.
#ifndef RWKV_RING_PRE
#define RWKV_RING_PRE 8
#endif
// TEST build only (tests/test_engine_gpu.py builds a variant with -DRWKV_TEST_DROP_GROUP=1): the loader "loses" every workgroup's last
// units, so the consumers' bounded wait must give up and the call must fail with RWKV_E_DEVICE instead of returning garbage
#ifndef RWKV_TEST_DROP_GROUP
#define RWKV_TEST_DROP_GROUP 0
#endif
#ifndef RWKV_RING_PRE_DEPTH
#define RWKV_RING_PRE_DEPTH 20
#endif
constexpr int NC = NW - 1;              // consumer waves of an LDS-DMA kernel (the last wave is the loader)

// ------------------------------------------------------------------------------------------
struct FirstArgs {
    const float *embed;   // [V][D] f32 (device resident), first stage only
    const double *ln;     // layernorm table; rows 0,1 = ln0 weight, bias
    double *x;            // residual stream [D]: written here
    const double *x_in;   // later pipeline stage: the residual vector handed over by the previous stage (may be x itself)
    SiteStatic st;        // ln1 site of this stage's first layer
    SiteDyn dy;
    const double *sxy;    // state xy of that layer
    size_t slot_stride;
    const Ctl *ctl;
    int D;
    int from_token;       // 1: x = ln0(embed[token]) (rwkv.cu:513-524); 0: x was handed over by the previous stage
};
// Produce the residual vector (first stage) and open the first layer's ln1 site.  A few workgroups,
// each owning a slice of the channels (every one recomputes the ln0 statistics of the 16 KB row).
__global__ __launch_bounds__(NT) void k_first(FirstArgs a)
{
    __shared__ double red[RED_BYTES / 8];
    const int D = a.D;
    const int j0 = block_lo(D), j1 = block_hi(D);
    const size_t so = (size_t)a.ctl->slot * a.slot_stride;
    double mean = 0.0, rstd = 1.0;
    const float *row = a.from_token ? a.embed + (size_t)a.ctl->token * D : nullptr;
    if (a.from_token) {
        double s[2] = {0.0, 0.0};
        for (int j = threadIdx.x; j < D; j += NT) { const double v = (double)row[j]; s[0] += v; s[1] += v * v; }
        block_sum<2>(s, red + RED_STATS);
        mean = s[0] / (double)D;
        rstd = 1.0 / sqrt((s[1] - s[0] * mean) / (double)(D - 1));
        __syncthreads();
    }
    SiteAcc<3> acc;
    acc.clear();
    for (int j = j0 + threadIdx.x; j < j1; j += NT) {
        double x;
        if (a.from_token) { x = a.ln[j] * (((double)row[j] - mean) * rstd) + a.ln[D + j]; a.x[j] = x; }
        else { x = a.x_in[j]; a.x[j] = x; }
        SitePre<3> pre;
        site_prefetch<3>(a.st, j, pre);
        site_emit<3>(pre, a.dy, D, j, x, a.sxy[so + j], acc);
    }
    site_publish<3, 64>(acc, a.dy, red);
}

// ------------------------------------------------------------------------------------------
struct AttArgs {
    const double *x;                      // residual stream [D]
    SiteStatic st;                        // ln1 site (3 vectors: k, v, r)
    SiteDyn dy;
    const uint8_t *w;                     // [D][3][D] u8: rows K_i, V_i, R_i of channel i
    const unsigned *rs;                   // [D][3] row sums of w (for the 2^22 limb offset)
    const double *uw, *ew;                // precomputed bonus+decay and exp(decay), [D]
    const float *r_att, *o_att;           // att_out scale / offset (to pre-scale the gated wkv)
    double *saa, *sbb;                    // state arrays [slots][L][D], already offset to this layer
    size_t slot_stride;                   // L*D
    float *ybuf;                          // [D] gated wkv * r_att (input vector of k_attout)
    double *partS;                        // [gridDim.x] partial sums of gated wkv * o_att
    float *partM;                         // [gridDim.x] partial max |ybuf| (k_attout's quantisation scale)
    const Ctl *ctl;
    int D;
    int ns;                               // tile form (tile.hip.h): LDS ring units
    unsigned long long *tl;               // optional phase timeline (see tl_stamp)
    unsigned *herr;                       // tile form: the context's error word (ring_report)
};

// The epilogue of one channel g of the K/V/R class, for both forms (k_att: inputs in registers; k_att_t, tile.hip.h: in its LDS stash): the
// WKV recurrence and the receptance gate (rwkv.cu:242-255) from k's two exponentials e1 = exp(u + w + k), ek = exp(k), the values v and r
// and the channel's state, decay and att_out constants.  Scalars, not a struct of everything: k_att_t has no registers to spare.  saa, sbb: the
// state arrays of the call's slot (as pointers, so that the slot's offset stays one scalar add per array: it is wave-uniform, g is not).
__device__ __forceinline__ void att_epilogue(double *saa, double *sbb, float *ybuf, int g, double aa, double bb, double e1, double ek, float v, float r, double ew, float ra, float oa, double &part, float &pmax)
{
    const double vv = (double)v;
    double y = (aa + e1 * vv) / (bb + e1);
    y = (1.0 / (1.0 + (double)expf(-r))) * y;       // rwkv.cu:250: exp of a float argument
    saa[g] = (aa + ek * vv) * ew;
    sbb[g] = (bb + ek) * ew;
    const float yf = (float)y;                       // att_out GEMV casts its input to f32 (rwkv.cu:290)
    const float ys = yf * ra;
    ybuf[g] = ys;
    part += (double)(yf * oa);
    pmax = fmaxf(pmax, fabsf(ys));
}

// ln1 site -> K,V,R dequant-GEMV -> WKV (rwkv.cu:535-545; kernels :351-392, :58-100, :221-259)
struct AttIn { unsigned rs[3]; double aa, bb, uw, ew; float ra, oa; };
template <int S>
__global__ __launch_bounds__(NT) void k_att(AttArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr RowLds L = RowGeo<1, S>::L;
    double *red = reinterpret_cast<double *>(smem + L.red);
    unsigned *xq = reinterpret_cast<unsigned *>(smem + L.xq);
    const int D = a.D, lane = threadIdx.x & 63, wave = wave_id();
    const int chunks = D >> 4;
    const int g0 = block_lo(D);
    const int g1 = block_hi(D);
    const size_t so = (size_t)a.ctl->slot * a.slot_stride;

    tl_stamp(a.tl, 0);
    // every wave requests its first groups, even one without work (it re-reads a neighbour's rows): a
    // branch around the loads would make hipcc's waitcnt pass drain the weights early
    auto base = [&](int g) { return a.w + (size_t)(g < g1 ? g : (g1 > g0 ? g1 - 1 : 0)) * 3 * D; };
    double sc[3];
    float S0, S1, S2;
    auto scalars = [&](const SiteRed<3> &sr) {
        sc[0] = scale_of(sr.amax[0]); sc[1] = scale_of(sr.amax[1]); sc[2] = scale_of(sr.amax[2]);
        S0 = (float)sr.S[0]; S1 = (float)sr.S[1]; S2 = (float)sr.S[2];
    };
    // channel g = one group of three rows (K, V, R); the wave that finished them runs the WKV recurrence and the
    // receptance gate of that channel at once (rwkv.cu:242-255): no staging of k/v/r, no pass after the last row
    double part = 0.0;
    float pmax = 0.f;
    auto pre = [&](int g) {
        AttIn in;
#pragma unroll
        for (int m = 0; m < 3; m++) in.rs[m] = a.rs[g * 3 + m];
        in.aa = a.saa[so + g]; in.bb = a.sbb[so + g]; in.uw = a.uw[g]; in.ew = a.ew[g];
        in.ra = a.r_att[g]; in.oa = a.o_att[g];
        return in;
    };
    auto epi = [&](int g, const unsigned long long (&T)[3], const AttIn &in) {
        if (lane == 0) {
            const float k = row_value(T[0], in.rs[0], sc[0]) + S0, v = row_value(T[1], in.rs[1], sc[1]) + S1;
            const float r = row_value(T[2], in.rs[2], sc[2]) + S2;
            att_epilogue(a.saa + so, a.sbb + so, a.ybuf, g, in.aa, in.bb, exp(in.uw + (double)k), exp((double)k), v, r, in.ew, in.ra, in.oa, part, pmax);
        }
    };
    u32x4 wA[3][S];
    int gA;
    unsigned *gctr = group_counter(red);
    first_groups(g0, wave, gctr, gA);   // the counter is visible behind the prologue's barriers
    SiteRed<3> sr;
    site_open<3, 3, S, (RWKV_SPLIT & 1) != 0>(a.st, a.dy, a.x, D, red, xq, wA, base(gA), (size_t)D, sr, true, a.tl);
    scalars(sr);
    stream_groups<3, S, PAT_PER_ROW>(wA, gA, g0, g1, gctr, xq, lane, (size_t)D, chunks, base, pre, epi);
    tl_stamp(a.tl, 6);
    __syncthreads();   // every wave is past its last read of the reduction scratch
    block_sum_max(part, pmax, red + RED_PART);
    if (threadIdx.x == 0) { a.partS[blockIdx.x] = part; a.partM[blockIdx.x] = pmax; }
    tl_stamp(a.tl, 7);
}

// ------------------------------------------------------------------------------------------
struct AttOutArgs {
    const uint8_t *w;      // [D][D] u8 rows = output channels
    const unsigned *rs;    // [D] row sums
    const float *ybuf;     // [D] pre-scaled input vector
    const double *partS;   // [n_part] partial offset sums (n_part <= NT)
    const float *partM;    // [n_part] partial max |ybuf|
    int n_part;
    double *x;             // residual stream, updated in place (row-owned)
    const double *lnw, *lnb;   // ln1 rows of this layer (f64): the state xy written here is ln1's output
    const double *lnstat;  // [2] mean, rstd of the ln1 site (published by k_att)
    double *sxy;           // state xy of this layer
    SiteStatic st;         // ln2 site (2 vectors) that this kernel opens for k_ffn_rk
    SiteDyn dy;
    const double *sdd;     // state dd of this layer (the ln2 site's prev)
    size_t slot_stride;
    const Ctl *ctl;
    int D;
    int ns;                // tile form (tile.hip.h): LDS ring units
    unsigned long long *tl;
    unsigned *herr;        // tile form: the context's error word (ring_report)
};

// The epilogue of one row mi of the att_out class, for both forms (k_attout; k_attout_t, tile.hip.h): the residual through f32 from the row's
// value val, the state xy, and the row's share of the ln2 site it opens (left in acc).  pre: the row's producer constants of that site, where the
// form holds them
__device__ __forceinline__ void attout_epilogue(const AttOutArgs &a, size_t so, int D, int mi, float val, double xold, double lw, double lb, double prev2, double mean1, double rstd1, const SitePre<2> &pre, SiteAcc<2> &acc)
{
    const float accf = (float)xold + val;                        // f32 accumulator pre-loaded with x (:548)
    const double xnew = (double)accf;                            // :553
    a.x[mi] = xnew;
    a.sxy[so + mi] = lw * ((xold - mean1) * rstd1) + lb;         // mixatt's state write (:385): ln1 output
    site_emit<2>(pre, a.dy, D, mi, xnew, prev2, acc);
}

// att_out dequant-GEMV + residual through f32 (rwkv.cu:548-553), R rows per group; commits state xy;
// opens the ln2 site for the rows it owns
template <int R> struct AttOutIn { unsigned rsum; double xold, lw, lb, prev2; SitePre<2> pre; int mi, shift; };
template <int S, int R>
__global__ __launch_bounds__(NT) void k_attout(AttOutArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr RowLds L = RowGeo<2, S>::L;
    double *red = reinterpret_cast<double *>(smem + L.red);
    unsigned *xq = reinterpret_cast<unsigned *>(smem + L.xq);
    const int D = a.D, lane = threadIdx.x & 63, wave = wave_id();
    const int chunks = D >> 4;
    tl_stamp(a.tl, 0);
    const int G = (D + R - 1) / R;
    const int g0 = block_lo(G);
    const int g1 = block_hi(G);

    const double mean1 = a.lnstat[0], rstd1 = a.lnstat[1];
    const size_t so = (size_t)a.ctl->slot * a.slot_stride;
    auto base = [&](int gg) {
        int row = (gg < g1 ? gg : (g1 > g0 ? g1 - 1 : 0)) * R;
        if (row > D - R) row = D - R;          // the last group may overlap the previous one
        return a.w + (size_t)row * D;
    };
    float Sf, amax;
    double sc;
    SiteAcc<2> acc;
    acc.clear();
    auto pre = [&](int g) {
        AttOutIn<R> in;
        int row0 = g * R;
        in.shift = (row0 > D - R) ? row0 - (D - R) : 0;
        row0 -= in.shift;
        in.mi = row0 + (lane < R ? lane : 0);               // lane r owns row row0 + r
        in.rsum = a.rs[in.mi];
        in.xold = a.x[in.mi]; in.lw = a.lnw[in.mi]; in.lb = a.lnb[in.mi]; in.prev2 = a.sdd[so + in.mi];
        site_prefetch<2>(a.st, in.mi, in.pre);
        return in;
    };
    auto epi = [&](int, const unsigned long long (&T)[R], const AttOutIn<R> &in) {
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (lane == r && r >= in.shift)
                attout_epilogue(a, so, D, in.mi, row_value(T[r], in.rsum, sc) + Sf, in.xold, in.lw, in.lb, in.prev2, mean1, rstd1, in.pre, acc);
        }
    };
    u32x4 wA[R][S];
    int gA;
    unsigned *gctr = group_counter(red);
    first_groups(g0, wave, gctr, gA);
    vec_open<1, R, S, (RWKV_SPLIT & 2) != 0>(a.ybuf, a.partS, a.partM, a.n_part, D, red, xq, wA, base(gA), (size_t)D, Sf, amax, a.tl);
    sc = scale_of(amax);
    stream_groups<R, S, PAT_SHARED>(wA, gA, g0, g1, gctr, xq, lane, (size_t)D, chunks, base, pre, epi);
    __syncthreads();   // every wave is past its last read of the reduction scratch (and of the staged vector)
    tl_stamp(a.tl, 6);
    site_publish<2, R>(acc, a.dy, xq);   // the staged vector is dead: its LDS is the scratch
    tl_stamp(a.tl, 7);
}

// ------------------------------------------------------------------------------------------
struct FfnRKArgs {
    const double *x;
    SiteStatic st;                    // ln2 site (2 vectors: ffn k, ffn r)
    SiteDyn dy;
    const uint8_t *w;                 // [D][5][D]: rows ffn_k out 4i..4i+3, then ffn_r out i
    const unsigned *rs;               // [D][5] row sums
    const float *r_fv, *o_fv;         // ffn_v scale / offset [4D]
    float *hbuf;                      // [4D] relu^2(k) * r_fv
    float *rgate;                     // [D] sigmoid(r)
    double *partS;                    // [gridDim.x]
    float *partM;                     // [gridDim.x] partial max |hbuf| (k_ffnv's quantisation scale)
    const Ctl *ctl;
    int D;
    int ns;                           // tile form (tile.hip.h): LDS ring units
    unsigned long long *tl;           // optional phase timeline (see tl_stamp)
    unsigned *herr;                   // tile form: the context's error word (ring_report)
};

// The epilogues of the ffn k/r class, for both forms (k_ffn_rk; k_ffn_rk_t, tile.hip.h), from a row's value val.  An ffn_k row (hidden unit i; rq / oq =
// ffn_v's scale / offset of that unit): relu^2, pre-scaled for ffn_v.  The ffn_r row of channel i: the gate.
__device__ __forceinline__ void ffn_k_epilogue(const FfnRKArgs &a, int i, float val, float rq, float oq, double &part, float &pmax)
{
    float h = val * (float)(val > 0.f);   // rwkv.cu:189-190
    h = h * h;
    const float hs = h * rq;
    a.hbuf[i] = hs;
    part += (double)(h * oq);
    pmax = fmaxf(pmax, fabsf(hs));
}
__device__ __forceinline__ void ffn_r_epilogue(const FfnRKArgs &a, int i, float val) { a.rgate[i] = (float)(1.0 / (1.0 + exp(-(double)val))); }   // rwkv.cu:212

// ln2 site -> ffn_r GEMV + sigmoid, ffn_k GEMV + relu^2 (rwkv.cu:557-573)
struct FfnRKIn { unsigned rsum; float rq, oq; };
template <int S>
__global__ __launch_bounds__(NT) void k_ffn_rk(FfnRKArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr RowLds L = RowGeo<3, S>::L;
    double *red = reinterpret_cast<double *>(smem + L.red);
    unsigned *xq = reinterpret_cast<unsigned *>(smem + L.xq);
    const int D = a.D, lane = threadIdx.x & 63, wave = wave_id();
    const int chunks = D >> 4;
    const int g0 = block_lo(D);
    const int g1 = block_hi(D);
    tl_stamp(a.tl, 0);

    auto base = [&](int g) { return a.w + (size_t)(g < g1 ? g : (g1 > g0 ? g1 - 1 : 0)) * 5 * D; };
    double sck, scr;
    float Sk, Sr;
    auto scalars = [&](const SiteRed<2> &sr) { sck = scale_of(sr.amax[0]); scr = scale_of(sr.amax[1]); Sk = (float)sr.S[0]; Sr = (float)sr.S[1]; };
    // channel g = the four ffn_k rows 4g..4g+3 and the ffn_r row g; lane q < 4 finishes hidden unit 4g + q (relu^2,
    // pre-scaled for ffn_v), lane 4 the receptance gate -- as soon as the group's sums exist
    double part = 0.0;
    float pmax = 0.f;
    auto pre = [&](int g) {
        FfnRKIn in;
        in.rsum = a.rs[g * 5 + (lane < 5 ? lane : 0)];
        const int kk = 4 * g + (lane < 4 ? lane : 0);
        in.rq = a.r_fv[kk]; in.oq = a.o_fv[kk];
        return in;
    };
    auto epi = [&](int g, const unsigned long long (&T)[5], const FfnRKIn &in) {
        float val = 0.f;     // lane r finishes row r (the sums are wave-uniform, the row sums per lane)
#pragma unroll
        for (int r = 0; r < 5; r++) {
            const float vr = row_value(T[r], in.rsum, r < 4 ? sck : scr) + (r < 4 ? Sk : Sr);
            val = lane == r ? vr : val;
        }
        if (lane < 4) ffn_k_epilogue(a, 4 * g + lane, val, in.rq, in.oq, part, pmax);
        else if (lane == 4) ffn_r_epilogue(a, g, val);
    };
    u32x4 wA[5][S];
    int gA;
    unsigned *gctr = group_counter(red);
    first_groups(g0, wave, gctr, gA);
    SiteRed<2> sr;
    site_open<2, 5, S, (RWKV_SPLIT & 4) != 0>(a.st, a.dy, a.x, D, red, xq, wA, base(gA), (size_t)D, sr, true, a.tl);
    scalars(sr);
    stream_groups<5, S, PAT_FFN_RK>(wA, gA, g0, g1, gctr, xq, lane, (size_t)D, chunks, base, pre, epi);
    tl_stamp(a.tl, 6);
    __syncthreads();   // every wave is past its last read of the reduction scratch
    block_sum_max(part, pmax, red + RED_PART);
    if (threadIdx.x == 0) { a.partS[blockIdx.x] = part; a.partM[blockIdx.x] = pmax; }
    tl_stamp(a.tl, 7);
}

// ------------------------------------------------------------------------------------------
struct FfnVArgs {
    const uint8_t *w;      // [D][4D] u8: row i = output channel i, as 4 quarter-rows of D bytes
    const unsigned *rs;    // [D] row sums (whole 4D row)
    const float *hbuf;     // [4D] pre-scaled hidden vector
    const double *partS;
    const float *partM;    // [n_part] partial max |hbuf|
    int n_part;
    const float *rgate;    // [D]
    double *x;             // residual stream (row-owned update)
    const double *lnw, *lnb;   // ln2 rows of this layer: the state dd written here is ln2's output
    const double *lnstat;  // [2] mean, rstd of the ln2 site (published by k_ffn_rk)
    double *sdd;
    SiteStatic st;         // the NEXT site: ln1 of layer l+1 (3 vectors) or ln_out -> head (1 vector)
    SiteDyn dy;
    const double *sprev;   // state xy of layer l+1 (prev of the next ln1 site); unused for the head site
    size_t slot_stride;
    const Ctl *ctl;
    int D;
    int ns;                // tile form (tile.hip.h): LDS ring units
    unsigned long long *tl;
    unsigned *herr;        // tile form: the context's error word (ring_report)
};

// The epilogue of one row g of the ffn_v class, for both forms (k_ffnv; k_ffnv_t, tile.hip.h): blockout from the row's value v and the gate rg,
// the state dd, and the row's share of the next site (left in acc; pre as in attout_epilogue)
template <int NVN>
__device__ __forceinline__ void ffnv_epilogue(const FfnVArgs &a, size_t so, int D, int g, float v, float rg, double xold, double lw, double lb, double prevn, double mean2, double rstd2, const SitePre<NVN> &pre, SiteAcc<NVN> &acc)
{
    const double xnew = xold + (double)(v * rg);                 // blockout, rwkv.cu:407 (f32 product)
    a.x[g] = xnew;
    a.sdd[so + g] = lw * ((xold - mean2) * rstd2) + lb;          // mixffn's state write (:344): ln2 output
    site_emit<NVN>(pre, a.dy, D, g, xnew, prevn, acc);
}

// ffn_v dequant-GEMV, x += v * sigmoid(r) (rwkv.cu:574-577); commits state dd; opens the next site
template <int NVN> struct FfnVIn { unsigned rsum; double xold, lw, lb, prevn; float rg; SitePre<NVN> pre; };
template <int S, int NVN>
__global__ __launch_bounds__(NT) void k_ffnv(FfnVArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr RowLds L = RowGeo<4, S>::L;
    double *red = reinterpret_cast<double *>(smem + L.red);
    unsigned *xq = reinterpret_cast<unsigned *>(smem + L.xq);
    const int D = a.D, lane = threadIdx.x & 63, wave = wave_id();
    const int chunks = D >> 4;
    tl_stamp(a.tl, 0);
    const int g0 = block_lo(D);
    const int g1 = block_hi(D);

    const double mean2 = a.lnstat[0], rstd2 = a.lnstat[1];
    const size_t so = (size_t)a.ctl->slot * a.slot_stride;
    auto base = [&](int g) { return a.w + (size_t)(g < g1 ? g : (g1 > g0 ? g1 - 1 : 0)) * 4 * D; };
    float Sf, amax;   // one scale for the whole 4D hidden vector
    double sc;
    SiteAcc<NVN> acc;
    acc.clear();
    auto pre = [&](int g) {
        FfnVIn<NVN> in;
        in.rsum = a.rs[g];
        in.xold = a.x[g]; in.lw = a.lnw[g]; in.lb = a.lnb[g];
        in.prevn = NVN == 3 ? a.sprev[so + g] : 0.0;
        in.rg = a.rgate[g];
        site_prefetch<NVN>(a.st, g, in.pre);
        return in;
    };
    auto epi = [&](int g, const unsigned long long (&T)[4], const FfnVIn<NVN> &in) {
        if (lane == 0)
            ffnv_epilogue<NVN>(a, so, D, g, row_value((T[0] + T[1]) + (T[2] + T[3]), in.rsum, sc) + Sf, in.rg, in.xold, in.lw, in.lb, in.prevn, mean2, rstd2, in.pre, acc);
    };
    u32x4 wA[4][S];
    int gA;
    unsigned *gctr = group_counter(red);
    first_groups(g0, wave, gctr, gA);
    vec_open<4, 4, S, (RWKV_SPLIT & 8) != 0>(a.hbuf, a.partS, a.partM, a.n_part, D, red, xq, wA, base(gA), (size_t)D, Sf, amax, a.tl);
    sc = scale_of(amax);
    stream_groups<4, S, PAT_PER_ROW>(wA, gA, g0, g1, gctr, xq, lane, (size_t)D, chunks, base, pre, epi);
    __syncthreads();   // every wave is past its last read of the reduction scratch
    tl_stamp(a.tl, 6);
    site_publish<NVN, 1>(acc, a.dy, xq);   // the staged vector is dead: its LDS is the scratch
    tl_stamp(a.tl, 7);
}

// ------------------------------------------------------------------------------------------
struct HeadArgs {
    const double *x;
    SiteStatic st;             // ln_out site (1 vector, no token shift)
    SiteDyn dy;
    const uint8_t *w;          // [V][D] u8
    const unsigned *rs;        // [V] row sums
    float *logits;             // [max_ctx][V]
    float *blk_val;            // [gridDim.x] per-workgroup max logit (index 0 banned)
    unsigned *blk_idx;         // [gridDim.x]
    const Ctl *ctl;
    int D;
};

// the greedy pick's order, shared by every argmax here: a larger logit wins, equal logits go to the lower id, and NaN never
// wins (every comparison with it is false)
__device__ __forceinline__ bool am_better(float v, unsigned i, float best, unsigned besti) { return v > best || (v == best && i < besti); }
// fold (best, besti) over the 64 lanes of a wave (every lane ends with the wave's winner)
__device__ __forceinline__ void am_wave_fold(float &best, unsigned &besti)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ov = __shfl_xor(best, m, 64);
        const unsigned oi = __shfl_xor(besti, m, 64);
        if (am_better(ov, oi, best, besti)) { best = ov; besti = oi; }
    }
}

// ln_out site -> head dequant-GEMV -> logits (rwkv.cu:585-589); also per-workgroup argmax partials
template <int R> struct HeadIn { unsigned rsr[R]; int row0, shift; };
template <int S, int R = RWKV_HEAD_R>
__global__ __launch_bounds__(NT) void k_head(HeadArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr RowLds L = RowGeo<5, S>::L;
    double *red = reinterpret_cast<double *>(smem + L.red);
    unsigned *xq = reinterpret_cast<unsigned *>(smem + L.xq);
    float *bval = reinterpret_cast<float *>(smem + L.bval);
    unsigned *bidx = reinterpret_cast<unsigned *>(smem + L.bidx);
    const int D = a.D, lane = threadIdx.x & 63, wave = wave_id();
    const int chunks = D >> 4;
    const int V = (int)VOCAB;
    const int G = (V + R - 1) / R;
    const int g0 = block_lo(G);
    const int g1 = block_hi(G);
    float *lg = a.logits + (size_t)a.ctl->out_row * V;     // read at entry: behind the prologue's barriers it is a cold load

    auto base = [&](int gg) {
        int row = (gg < g1 ? gg : (g1 > g0 ? g1 - 1 : 0)) * R;
        if (row > V - R) row = V - R;
        return a.w + (size_t)row * D;
    };
    float Sf;
    double sc;
    float best = -INFINITY;
    unsigned besti = 0xffffffffu;
    auto pre = [&](int g) {
        HeadIn<R> in;
        in.row0 = g * R;
        in.shift = (in.row0 > V - R) ? in.row0 - (V - R) : 0;
        in.row0 -= in.shift;
#pragma unroll
        for (int r = 0; r < R; r++) in.rsr[r] = a.rs[in.row0 + r];
        return in;
    };
    auto epi = [&](int, const unsigned long long (&T)[R], const HeadIn<R> &in) {
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int i = in.row0 + r;
            const float val = row_value(T[r], in.rsr[r], sc) + Sf;
            if (lane == r && r >= in.shift) lg[i] = val;
            if (i != 0 && am_better(val, (unsigned)i, best, besti)) { best = val; besti = (unsigned)i; }
        }
    };
    u32x4 wA[R][S];
    int gA;
    unsigned *gctr = group_counter(red);
    first_groups(g0, wave, gctr, gA);
    SiteRed<1> sr;
    site_open<1, R, S, (RWKV_SPLIT & 16) != 0>(a.st, a.dy, a.x, D, red, xq, wA, base(gA), (size_t)D, sr, false, nullptr);
    Sf = (float)sr.S[0]; sc = scale_of(sr.amax[0]);
    stream_groups<R, S, PAT_SHARED>(wA, gA, g0, g1, gctr, xq, lane, (size_t)D, chunks, base, pre, epi);
    if (lane == 0) { bval[wave] = best; bidx[wave] = besti; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < NW; i++)
            if (am_better(bval[i], bidx[i], best, besti)) { best = bval[i]; besti = bidx[i]; }
        a.blk_val[blockIdx.x] = best;
        a.blk_idx[blockIdx.x] = besti;
    }
}

// finish the greedy pick: argmax over workgroup partials (ties -> lowest id), feed it back as the
// next token and append it to the generated-id list.  One 64-lane wave.
__global__ void k_argmax_finish(const float *blk_val, const unsigned *blk_idx, int n, Ctl *ctl,
                                unsigned long long *gen, unsigned gen_cap)
{
    float best = -INFINITY;
    unsigned besti = 0xffffffffu;
    for (int i = threadIdx.x; i < n; i += 64) {
        const float v = blk_val[i];
        const unsigned id = blk_idx[i];
        if (am_better(v, id, best, besti)) { best = v; besti = id; }
    }
    am_wave_fold(best, besti);
    if (threadIdx.x == 0) {
        // all-NaN / all -inf logits leave no winner (the reference's un-stabilised WKV can overflow with unusual
        // weights): feed token 0 like the sampler's fallback instead of indexing the embedding out of bounds
        if (besti >= VOCAB) besti = 0u;
        const unsigned st = ctl->step;
        if (st < gen_cap) gen[st] = besti;
        ctl->token = besti;
        ctl->step = st + 1;
    }
}

// ---- the greedy pick over N logits rows (batched decode, rwkv_decode_batch_greedy) ----
// k_argmax_rows, grid (AM_SLICES, rows): workgroup (p, r) scans slice p of row r's 16-byte aligned body with float4 loads -- a row is
// 201 108 bytes, so row r starts 4 r bytes past a 16-byte boundary -- and slice 0 also the <= 3 elements in front of the body and the
// <= 3 behind it; id 0 is banned as in k_head.  A (slice, row) grid keeps every CU busy (16 x 32 workgroups at N = 32) where one
// workgroup per row would leave most of them idle.  k_argmax_rows_finish, one wave per row: folds the row's partials into ids[r]
// (no winner -- all logits NaN -- gives token 0, as k_argmax_finish).
constexpr int AM_SLICES = 16;
constexpr int AM_NT = 256;
static_assert(AM_SLICES <= 64, "one lane per partial in the finish");
__global__ __launch_bounds__(AM_NT) void k_argmax_rows(const float *__restrict__ logits, float *__restrict__ part_val, unsigned *__restrict__ part_idx)
{
    __shared__ float sv[AM_NT / 64];
    __shared__ unsigned si[AM_NT / 64];
    const int V = (int)VOCAB;
    const float *lg = logits + (size_t)blockIdx.y * V;
    const int h = (int)(((16u - ((unsigned)(uintptr_t)lg & 15u)) & 15u) >> 2);   // elements in front of the first 16-byte boundary
    const int nv = (V - h) >> 2;                                                  // float4s of the aligned body
    const f32x4 *body = reinterpret_cast<const f32x4 *>(lg + h);
    float best = -INFINITY;
    unsigned besti = 0xffffffffu;
    const int v1 = block_hi(nv);
#pragma unroll 4
    for (int v = block_lo(nv) + (int)threadIdx.x; v < v1; v += AM_NT) {      // ~3 float4 per thread: all of them in flight
        const f32x4 q = body[v];
        const unsigned i = (unsigned)(h + 4 * v);
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (i + k != 0u && am_better(q[k], i + k, best, besti)) { best = q[k]; besti = i + k; }
    }
    if (blockIdx.x == 0 && threadIdx.x < 8) {      // head [0, h) on threads 0..3, tail [h + 4 nv, V) on threads 4..7
        const int i = threadIdx.x < 4 ? (int)threadIdx.x : h + 4 * nv + (int)threadIdx.x - 4;
        if (i != 0 && i < (threadIdx.x < 4 ? h : V) && am_better(lg[i], (unsigned)i, best, besti)) { best = lg[i]; besti = (unsigned)i; }
    }
    am_wave_fold(best, besti);
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = best; si[threadIdx.x >> 6] = besti; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < AM_NT / 64; w++)
            if (am_better(sv[w], si[w], best, besti)) { best = sv[w]; besti = si[w]; }
        part_val[blockIdx.y * AM_SLICES + blockIdx.x] = best;
        part_idx[blockIdx.y * AM_SLICES + blockIdx.x] = besti;
    }
}
__global__ __launch_bounds__(64) void k_argmax_rows_finish(const float *__restrict__ part_val, const unsigned *__restrict__ part_idx, unsigned long long *__restrict__ ids)
{
    const int lane = threadIdx.x;
    float best = -INFINITY;
    unsigned besti = 0xffffffffu;
    if (lane < AM_SLICES) { best = part_val[blockIdx.x * AM_SLICES + lane]; besti = part_idx[blockIdx.x * AM_SLICES + lane]; }
    am_wave_fold(best, besti);
    if (lane == 0) ids[blockIdx.x] = besti < VOCAB ? besti : 0u;
}

// ------------------------------------------------------------------------------------------
// Load-time re-tile: file layout src[N][M] (output index k contiguous, rwkv.cu:290 indexing
// w[j*M + k]) -> row-per-output dst[row(k)][N] with row(k) = (k/G)*RS + k%G + off.
__global__ void k_retile(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int N, int M,
                         int G, int RS, int off)
{
    __shared__ uint8_t tile[64][65];
    const int k0 = blockIdx.x * 64, j0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;   // 256 threads: 64 x 4
    for (int jj = ty; jj < 64; jj += 4) {
        const int j = j0 + jj, k = k0 + tx;
        tile[jj][tx] = (j < N && k < M) ? src[(size_t)j * M + k] : 0;
    }
    __syncthreads();
    for (int kk = ty; kk < 64; kk += 4) {
        const int k = k0 + kk, j = j0 + tx;
        if (k < M && j < N) {
            const size_t row = (size_t)(k / G) * RS + (k % G) + off;
            dst[row * N + j] = tile[tx][kk];
        }
    }
}

// row sums of a re-tiled matrix: rs[row] = sum_j w_t[row][j]; one wave per row (load time)
__global__ void k_rowsum(const uint8_t *__restrict__ w_t, unsigned *__restrict__ rs, size_t rows, int N)
{
    const size_t row = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const u32x4 *p = reinterpret_cast<const u32x4 *>(w_t + row * (size_t)N);
    unsigned acc = 0;
    for (int c = lane; c < (N >> 4); c += 64) {
        const u32x4 v = p[c];
#pragma unroll
        for (int q = 0; q < 4; q++) acc = __builtin_amdgcn_udot4(v[q], 0x01010101u, acc, false);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if (lane == 0) rs[row] = acc;
}

// uw = bonus + decay, ew = exp(decay)   (constants of rwkv.cu:247-252, hoisted out of the token loop)
__global__ void k_prep_wkv(const double *decay, const double *bonus, double *uw, double *ew, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { uw[i] = bonus[i] + decay[i]; ew[i] = exp(decay[i]); }
}

// Load-time tables of vector m of one LayerNorm site (see "LayerNorm sites" above): consumer side
// C[m][j] = r mix lnw; producer side P[j][PW] holds BL = r mix lnb, BP = r (1 - mix) and the same
// with the offset o in place of the scale r (Co, BoL, BoP) at [m*5 + 0..4].  mix == nullptr means
// no token shift (ln_out -> head).  Products are formed in f64 and stored as f32.  TC[m] = sum of the
// stored Co, maxC[m] = max |C|.  One workgroup per call.
__global__ __launch_bounds__(NT) void k_site_static(const double *lnw, const double *lnb, const double *mix, const float *r, const float *o,
                                                    float *C, float *P, double *TC, float *maxC, int m, int PW, int D)
{
    __shared__ double red[RED_BYTES / 8];
    double s[1] = {0.0};
    float mx[1] = {0.f};
    for (int j = threadIdx.x; j < D; j += NT) {
        const double mk = mix ? mix[j] : 1.0, rr = (double)r[j], oo = (double)o[j];
        const float c = (float)(rr * mk * lnw[j]), co = (float)(oo * mk * lnw[j]);
        C[(size_t)m * D + j] = c;
        float *pp = P + (size_t)j * PW + m * 5;
        pp[0] = (float)(rr * mk * lnb[j]);
        pp[1] = (float)(rr * (1.0 - mk));
        pp[2] = co;
        pp[3] = (float)(oo * mk * lnb[j]);
        pp[4] = (float)(oo * (1.0 - mk));
        s[0] += (double)co;
        mx[0] = fmaxf(mx[0], fabsf(c));
    }
    block_sum<1>(s, red + RED_STATS);
    block_max<1>(mx, red + RED_MAX);
    if (threadIdx.x == 0) { TC[m] = s[0]; maxC[m] = mx[0]; }
}

} // namespace rwkvk
