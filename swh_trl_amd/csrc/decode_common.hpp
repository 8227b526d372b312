// What the decode-step sources share (decode_gemm.hip, lm_head.hip, attn_decode.hip and
// the host side of wide_gemm.hip): vector types, the epilogue selector, the phase-stamp
// macro of the probe builds, the RMSNorm / pack helpers, the weight-fragment loads, the
// LDS layout of the X image, the fused sampler's argument structs, and the declarations
// of the host functions one source calls in another.  Internal; the public header is
// include/swh_trl_amd.h.
#pragma once

#include "common.hpp"

namespace swh {
// csrc/wide_gemm.hip: 1 = shape not eligible, else a SWH status
int wide_gemm(const void *x, const void *w, int64_t M, int64_t N, int64_t K, float eps, const float *ss_in,
              const void *bias, void *residual, int32_t silu, void *y, int64_t ldy, float *ss_out, void *workspace,
              int64_t workspace_bytes, int64_t counter_bytes, int32_t packed, hipStream_t stream);
int64_t wide_gemm_slab_bytes(int64_t M, int64_t N, int64_t K, int32_t silu);
bool wide_gemm_eligible(int64_t M, int64_t N, int64_t K, int32_t silu);
int wide_pack(const void *src, const void *norm_w, int64_t N, int64_t K, int32_t silu, void *dst, hipStream_t stream);
int wide_lm_sample(const void *x, const void *w, int64_t M, int64_t V, int64_t K, float eps, const float *ss_in,
                   const swh_sample_params &p, const uint64_t *rng, const int32_t *step, LmPart *part, int *pstride,
                   hipStream_t stream);
int frag_pack(const void *src, const void *norm_w, int64_t N, int64_t K, int32_t silu, void *dst, hipStream_t stream);
// csrc/lm_head.hip: the tile kernel for plain / bias (Bs non-null) / SiLU epilogues (epi: EPI_PLAIN, EPI_SILU)
int tile_gemm(int epi, int nm, dim3 grid, size_t lds, hipStream_t s, const uint16_t *X, const uint16_t *W, int M, int N,
              int K, const uint16_t *NWt, float eps, const float *ss_in, const uint16_t *Bs, uint16_t *Y, int ldy,
              int fw, int yf);

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int64_t kCounterBytes = 1 << 16;  // split-K ticket counters (16384 tiles)

enum : int { EPI_PLAIN = 0, EPI_RESIDUAL = 1, EPI_SILU = 2 };

// Phase timestamps for tools/gemm_probe (a build with SWH_GEMM_TRACE_ON defined):
// wall clock (100 MHz) of wave 0 at each phase boundary, per workgroup.
#ifdef SWH_GEMM_TRACE_ON
__device__ unsigned long long *g_gemm_trace;
#define SWH_GEMM_TRACE(i)                                                                                      \
    if (threadIdx.x == 0 && g_gemm_trace)                                                                      \
    g_gemm_trace[((int64_t)(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 8 + (i)] =        \
        wall_clock64()
#else
#define SWH_GEMM_TRACE(i)
#endif

// Workgroup barrier that waits for LDS traffic only: global loads issued
// before it stay in flight (the compiler's counted vmcnt waits cover uses).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ bf16x8 as_bf16x8(const uint4 &v) { return __builtin_bit_cast(bf16x8, v); }

// Normalised X: bf16(w * bf16(x * rstd)) for 8 consecutive k (Qwen2RMSNorm's
// two roundings), packed f32 math: 4 VALU per element.
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t norm_pair(uint32_t xv, f32x2 w, float rs) {
    const f32x2 xf = {__uint_as_float(xv << 16), __uint_as_float(xv & 0xffff0000u)};
    const uint32_t tb = __builtin_bit_cast(uint32_t, __builtin_convertvector(xf * rs, bf16x2));
    const f32x2 tf = {__uint_as_float(tb << 16), __uint_as_float(tb & 0xffff0000u)};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(tf * w, bf16x2));
}
__device__ __forceinline__ uint4 norm_frag(const uint4 &xv, const float4 &w0, const float4 &w1, float rs) {
    return uint4{norm_pair(xv.x, f32x2{w0.x, w0.y}, rs), norm_pair(xv.y, f32x2{w0.z, w0.w}, rs),
                 norm_pair(xv.z, f32x2{w1.x, w1.y}, rs), norm_pair(xv.w, f32x2{w1.z, w1.w}, rs)};
}

__device__ __forceinline__ uint4 pack8(const float *v) {
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        o[k] = (uint32_t)f32_to_bf16_bits(v[2 * k]) | ((uint32_t)f32_to_bf16_bits(v[2 * k + 1]) << 16);
    return uint4{o[0], o[1], o[2], o[3]};
}

// one 16-B weight fragment (read once per launch)
__device__ __forceinline__ uint4 ld_w(const uint16_t *p) { return *reinterpret_cast<const uint4 *>(p); }
// the same with the non-temporal policy chosen per kernel: the gate/up tiles (fragment-order
// weights, whole 1 KB runs per load) gain from it (11.15 -> 10.7 us), while the projections
// whose weights the attention launch warms into the Infinity Cache (qkv, o, down) and the
// lm-head sampler lose (profiles/r5_wnt_ab.log, r5_gunt_ab.log)
template <bool NT>
__device__ __forceinline__ uint4 ld_wt(const uint16_t *p) {
    if constexpr (NT) return ld_nt(reinterpret_cast<const uint4 *>(p));
    return ld_w(p);
}

// LDS layout of the GEMM kernel (bytes; host and device compute it alike):
//   [0,256) rstd[64] | [256,272) flag | [512, ...) norm-weight slice (f32)
//   | RMSNorm partials [MR][K/64] f32 | the X image [MR][Kr*2+16 B] (LDS-DMA);
//     the merge slots [NW/2][NB][MR+4] f32 reuse the image, or follow it when
//     the workgroup loops over several column blocks (the image must persist).
struct GemmLds {
    int64_t nw_off, ss_off, body_off, xs_bytes, slots_off, total;
};
// nm: 0 = plain X, 1 = RMSNorm applied to the X image, 2 = rstd row scale in the epilogue
// cb: the tile's 16-column blocks; wn: column groups of waves (nw / wn waves split K in each)
// (used: keeps the compiler from specialising this function for a source whose callers all
// pass the same constants — lm_head.hip: cb 1, mr 64, no persist — which re-associates the
// tile kernel's LDS offsets; with it the kernels compile as they did from one source)
__host__ __device__ __attribute__((used)) inline GemmLds gemm_lds(int cb, int mr, int nw, int krmax, int K, int nm, bool persist,
                                            int wn = 1) {
    GemmLds L;
    L.nw_off = 512;
    L.ss_off = L.nw_off + (nm == 1 ? (int64_t)krmax * 4 : 0);  // norm weights as f32
    L.body_off = L.ss_off + (nm ? ((int64_t)mr * (K / 64) * 4 + 15) / 16 * 16 : 0);  // partials beside the DMA'd image
    L.xs_bytes = (int64_t)mr * (krmax * 2 + 16);
    const int wk = nw / wn;
    const int64_t slots = (int64_t)(wk + 1) * 16 * cb * (mr + 4) * 4;  // [WK + 1][NB][MR+4]
    L.slots_off = L.body_off + (persist ? L.xs_bytes : 0);
    int64_t end = L.body_off + L.xs_bytes;
    if (L.slots_off + slots > end) end = L.slots_off + slots;
    L.total = end;
    return L;
}

constexpr int kLmMaxKS = 32;  // the tile kernel's K limit in k-steps: K <= 1024

// Fused sampler (SAMPLE): instead of storing logits, each wave folds its
// tiles into per-row Gumbel-max bests (the unfiltered swh_sample_step: EOS
// suppression, temperature, greedy) and writes one partial per row; the
// Philox block at counter {col, row >> 2} holds the four rows a lane owns.
struct LmSample {
    swh_sample_params p;
    const uint64_t *rng;
    const int32_t *step;
    LmPart *part;  // [M][pstride]
    int pstride;
    int fw = 0;    // weights in the swh_frag_pack layout (tile t = 16-row group t)
    int yf = 0;    // SiLU output in the fragment order down_proj's A operand reads (N % 32 == 0)
    float2 *lpart = nullptr;  // log-prob variants: [M][pstride] (max, sum e^(z - max)) of the processed scores
};

// The next step's input, produced by the finalize (swh_lm_head_sample_step):
// the drawn token's embedding row and its RMSNorm partial sums, and the step
// counter advanced by the last row to finish (ticket) — the three small
// launches embed_gather / step_advance / finalize become one.
struct LmNext {
    const uint16_t *embed;  // [V, H] (null: no gather, no advance)
    uint16_t *x;            // [M, H]
    float *ss;              // [M, H / 16] (nullable)
    int32_t *step;          // advanced once every row has read it
    int32_t *ticket;        // zero at allocation, self-resetting
    int H, M;
};

}  // namespace
}  // namespace swh
