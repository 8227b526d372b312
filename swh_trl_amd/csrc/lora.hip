// LoRA adapter kernels (gfx950): the rank-r products beside a frozen Linear
// W [N, K] — adapter A [Rp, K] and Bt [Rp, N] (B stored transposed), Rp = r
// rounded up to 16, pad rows zero.  bf16 operands, fp32 accumulation on
// v_mfma_f32_16x16x32_bf16 (lane l: A[row l & 15][k = 8 (l >> 4) + j],
// B[k = 8 (l >> 4) + j][col l & 15], D[row 4 (l >> 4) + reg][col l & 15]).
//
//   lora_down    u[T, Rp]  = x[T, K] M[Rp, K]^T        rank = MFMA rows, tokens = columns
//   lora_up_add  y[T, C]  += s u[T, Rp] M[Rp, C]       rank = MFMA k (zero-extended to 32)
//   lora_grad    G[Rp, C] += s u[T, Rp]^T in[T, C]     rank = MFMA rows, tokens = k
//   lora_merge   out[N, K] = bf16(W + s Bt^T A)        lora_up_add with u = Bt^T, per job
//
// Nothing here uses atomics: every output element has one owner and every
// reduction a fixed order, so two runs give the same bits.
#include "common.hpp"

namespace swh {
namespace {

typedef __bf16 bf16x8l __attribute__((ext_vector_type(8)));
typedef float f32x4l __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bf16x8l frag(const uint4 &v) { return __builtin_bit_cast(bf16x8l, v); }
__device__ __forceinline__ f32x4l mfma(const uint4 &a, const uint4 &b, const f32x4l &c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(a), frag(b), c, 0, 0, 0);
}
__device__ __forceinline__ uint32_t pack2(uint32_t lo, uint32_t hi) { return (lo & 0xffffu) | (hi << 16); }

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline int rank_pad(int r) { return (r + 15) / 16 * 16; }

// ---- lora_down ---------------------------------------------------------------
// One workgroup per 16 tokens; its four waves take the 32-wide k steps round
// robin (the activation row is read once, 16 B per lane) and wave 0 adds the
// four partial tiles in wave order.  M's rows are the MFMA rows, so a lane ends
// with four consecutive ranks of one token: one 8-byte store.  Columns >= r of u
// are written as zero whatever M's pad rows hold.
template <int RT>
__global__ __launch_bounds__(256) void lora_down_kernel(const uint16_t *__restrict__ x, const uint16_t *__restrict__ M,
                                                        uint16_t *__restrict__ u, int64_t T, int64_t K, int r,
                                                        int64_t ldx, int64_t ldm, int64_t ldu) {
    __shared__ float red[3][RT][4][64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int n = lane & 15, g = lane >> 4;
    const int64_t t0 = (int64_t)blockIdx.x * 16;
    const int64_t tok = t0 + n;
    const uint16_t *xr = x + (tok < T ? tok : T - 1) * ldx + 8 * g;  // rows past T read row T - 1, never stored
    const uint16_t *mr = M + (int64_t)n * ldm + 8 * g;
    f32x4l acc[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[rt] = f32x4l{0.f, 0.f, 0.f, 0.f};
    const int64_t ksteps = K / 32;
#pragma unroll 2
    for (int64_t ks = wid; ks < ksteps; ks += 4) {
        const uint4 xb = *reinterpret_cast<const uint4 *>(xr + ks * 32);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const uint4 ma = *reinterpret_cast<const uint4 *>(mr + (int64_t)rt * 16 * ldm + ks * 32);
            acc[rt] = mfma(ma, xb, acc[rt]);
        }
    }
    if (wid > 0) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int q = 0; q < 4; ++q) red[wid - 1][rt][q][lane] = acc[rt][q];
    }
    __syncthreads();
    if (wid != 0 || tok >= T) return;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        uint32_t b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float v = acc[rt][q];
#pragma unroll
            for (int w = 0; w < 3; ++w) v += red[w][rt][q][lane];
            b[q] = (rt * 16 + 4 * g + q < r) ? f32_to_bf16_bits(v) : 0u;
        }
        *reinterpret_cast<uint2 *>(u + tok * ldu + rt * 16 + 4 * g) = uint2{pack2(b[0], b[1]), pack2(b[2], b[3])};
    }
}

// ---- lora_up_add / lora_merge ------------------------------------------------
// A wave owns 16 tokens x 64 columns.  M is the MFMA A operand with its rows
// permuted: row i of tile t is column 16 (i >> 2) + 4 t + (i & 3) of the span, so
// lane group g = l >> 4 ends with columns 16 g .. 16 g + 15 of its token across
// the four tiles: y moves as two 16-byte pieces per lane, 128 contiguous bytes
// per token row.  The rank is the k dimension, zero-extended to 32 per step.
// The workgroup's four waves share the M tile through LDS and walk the token
// tiles round robin.
constexpr int kUpTok = 512;  // tokens per workgroup

template <int KS>
struct UpFrags {
    uint4 a[KS][4];
};

// M tile [KS * 32][64] into LDS: rows >= Rp and columns >= C are zero
template <int KS>
__device__ __forceinline__ void up_stage_m(uint16_t (*mt)[64], const uint16_t *__restrict__ M, int64_t ldm, int Rp,
                                           int64_t c0, int64_t C) {
    for (int v = threadIdx.x; v < KS * 32 * 8; v += 256) {
        const int row = v >> 3, cv = (v & 7) * 8;
        uint4 val = uint4{0u, 0u, 0u, 0u};
        if (row < Rp && c0 + cv < C) val = *reinterpret_cast<const uint4 *>(M + (int64_t)row * ldm + c0 + cv);
        *reinterpret_cast<uint4 *>(&mt[row][cv]) = val;
    }
}

template <int KS>
__device__ __forceinline__ void up_load_frags(UpFrags<KS> &f, const uint16_t (*mt)[64], int n, int g) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int cc = 16 * (n >> 2) + 4 * t + (n & 3);
            uint32_t e[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) e[j] = mt[ks * 32 + 8 * g + j][cc];
            f.a[ks][t] = uint4{pack2(e[0], e[1]), pack2(e[2], e[3]), pack2(e[4], e[5]), pack2(e[6], e[7])};
        }
}

// dst[16 columns] = bf16(src + s acc) for one lane: fp32 sum, one rounding; an
// element whose update is zero keeps its bits
__device__ __forceinline__ void up_epilogue(const uint16_t *src, uint16_t *dst, const f32x4l (&acc)[4], float s) {
    const uint4 y0 = *reinterpret_cast<const uint4 *>(src), y1 = *reinterpret_cast<const uint4 *>(src + 8);
    const uint32_t w[8] = {y0.x, y0.y, y0.z, y0.w, y1.x, y1.y, y1.z, y1.w};
    uint32_t o[8];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t word = w[2 * t + h];
            const uint32_t lo = word & 0xffffu, hi = word >> 16;
            const float a0 = acc[t][2 * h], a1 = acc[t][2 * h + 1];
            const uint32_t n0 = a0 == 0.f ? lo : f32_to_bf16_bits(fmaf(s, a0, bf16_bits_to_f32(lo)));
            const uint32_t n1 = a1 == 0.f ? hi : f32_to_bf16_bits(fmaf(s, a1, bf16_bits_to_f32(hi)));
            o[2 * t + h] = pack2(n0, n1);
        }
    *reinterpret_cast<uint4 *>(dst) = uint4{o[0], o[1], o[2], o[3]};
    *reinterpret_cast<uint4 *>(dst + 8) = uint4{o[4], o[5], o[6], o[7]};
}

template <int KS>
__global__ __launch_bounds__(256) void lora_up_add_kernel(const uint16_t *__restrict__ u,
                                                          const uint16_t *__restrict__ M, uint16_t *__restrict__ y,
                                                          int64_t T, int64_t C, int Rp, int64_t ldu, int64_t ldm,
                                                          int64_t ldy, float s) {
    __shared__ __attribute__((aligned(16))) uint16_t mt[KS * 32][64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int n = lane & 15, g = lane >> 4;
    const int64_t c0 = (int64_t)blockIdx.x * 64;
    up_stage_m<KS>(mt, M, ldm, Rp, c0, C);
    __syncthreads();
    UpFrags<KS> f;
    up_load_frags<KS>(f, mt, n, g);
    const int64_t tb0 = (int64_t)blockIdx.y * kUpTok;
    const int64_t tb1 = tb0 + kUpTok < T ? tb0 + kUpTok : T;
    const bool cols_ok = c0 + 16 * g < C;  // C % 16 == 0: a lane's 16 columns are all inside or all outside
    for (int64_t t0 = tb0 + 16 * wid; t0 < tb1; t0 += 64) {
        const int64_t tok = t0 + n;
        const uint16_t *ur = u + (tok < T ? tok : T - 1) * ldu;
        f32x4l acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = f32x4l{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int k = ks * 32 + 8 * g;
            uint4 ub = uint4{0u, 0u, 0u, 0u};
            if (k < Rp) ub = *reinterpret_cast<const uint4 *>(ur + k);
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = mfma(f.a[ks][t], ub, acc[t]);
        }
        if (tok < T && cols_ok) {
            uint16_t *yp = y + tok * ldy + c0 + 16 * g;
            up_epilogue(yp, yp, acc, s);
        }
    }
}

// One merge job: out [N, K] = bf16(W + scale Bt^T A), every matrix contiguous.
// tile0 = the job's first workgroup in the launch (prefix sum of the jobs' tiles).
struct MergeJob {
    const uint16_t *W, *A, *Bt;
    uint16_t *out;
    int64_t N, K, r, tile0;
    double scale;
};
constexpr int kMergeMaxJobs = 256, kMergeRows = 256;  // weight rows per workgroup (64 per wave)

__host__ __device__ inline int64_t merge_tiles(int64_t N, int64_t K) {
    return ((N + kMergeRows - 1) / kMergeRows) * ((K + 63) / 64);
}

template <int KS>
__device__ __forceinline__ void merge_tile(const MergeJob &jb, int64_t tile, uint16_t (*mt)[64]) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int n = lane & 15, g = lane >> 4;
    const int Rp = ((int)jb.r + 15) / 16 * 16;
    const int64_t ctiles = (jb.K + 63) / 64;
    const int64_t c0 = (tile % ctiles) * 64, r0 = (tile / ctiles) * kMergeRows;
    up_stage_m<KS>(mt, jb.A, jb.K, Rp, c0, jb.K);
    __syncthreads();
    UpFrags<KS> f;
    up_load_frags<KS>(f, mt, n, g);
    const float s = (float)jb.scale;
    const bool cols_ok = c0 + 16 * g < jb.K;
    const int64_t r1 = r0 + kMergeRows < jb.N ? r0 + kMergeRows : jb.N;
    for (int64_t t0 = r0 + 16 * wid; t0 < r1; t0 += 64) {
        const int64_t row = t0 + n;
        const int64_t rc = row < jb.N ? row : jb.N - 1;
        f32x4l acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = f32x4l{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int k = ks * 32 + 8 * g;
            uint32_t e[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) e[j] = (k + j < Rp) ? (uint32_t)jb.Bt[(int64_t)(k + j) * jb.N + rc] : 0u;
            const uint4 ub = uint4{pack2(e[0], e[1]), pack2(e[2], e[3]), pack2(e[4], e[5]), pack2(e[6], e[7])};
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = mfma(f.a[ks][t], ub, acc[t]);
        }
        if (row < jb.N && cols_ok) {
            const int64_t o = row * jb.K + c0 + 16 * g;
            up_epilogue(jb.W + o, jb.out + o, acc, s);
        }
    }
}

__global__ __launch_bounds__(256) void lora_merge_kernel(const MergeJob *__restrict__ jobs, int njobs) {
    __shared__ __attribute__((aligned(16))) uint16_t mt[64][64];
    __shared__ int64_t first[kMergeMaxJobs];
    for (int j = threadIdx.x; j < njobs; j += blockDim.x) first[j] = jobs[j].tile0;
    __syncthreads();
    const int64_t tile = blockIdx.x;
    int lo = 0, hi = njobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first[mid] <= tile) lo = mid;
        else hi = mid - 1;
    }
    const MergeJob jb = jobs[lo];
    const int64_t local = tile - jb.tile0;
    if (local < 0 || local >= merge_tiles(jb.N, jb.K) || jb.r < 1 || jb.r > 64) return;  // uniform per workgroup
    if (jb.r <= 32) merge_tile<1>(jb, local, mt);
    else merge_tile<2>(jb, local, mt);
}

// ---- lora_grad ---------------------------------------------------------------
// part[chunk][Rp][C] (fp32) = u[chunk's tokens]^T in[chunk's tokens], chunks of
// kGradChunk tokens summed in token order; lora_grad_fold then adds the chunks
// in order: G += s sum.  A workgroup takes 64 columns of one chunk; each
// 32-token step's u and `in` tiles go through LDS (16-byte global loads, the
// next step's issued before this step's MFMAs), because both MFMA operands need
// eight TOKENS of one column per lane.  Wave w owns columns 16 w .. 16 w + 15.
constexpr int kGradChunk = 1024;

template <int RT>
__global__ __launch_bounds__(256) void lora_grad_partial_kernel(const uint16_t *__restrict__ u,
                                                                const uint16_t *__restrict__ in,
                                                                float *__restrict__ part, int64_t T, int64_t C,
                                                                int64_t ldu, int64_t ldin) {
    constexpr int Rp = RT * 16;
    __shared__ __attribute__((aligned(16))) uint16_t su[2][32][Rp + 8];
    __shared__ __attribute__((aligned(16))) uint16_t sx[2][32][64 + 8];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int n = lane & 15, g = lane >> 4;
    const int64_t c0 = (int64_t)blockIdx.x * 64;
    const int64_t tb0 = (int64_t)blockIdx.y * kGradChunk;
    const int64_t tb1 = tb0 + kGradChunk < T ? tb0 + kGradChunk : T;
    const int xrow = tid >> 3, xcol = (tid & 7) * 8;  // this thread's piece of the `in` tile
    const bool xcol_ok = c0 + xcol < C;
    constexpr int UV = Rp / 8;                          // 16-byte pieces per u row
    const int urow = tid / UV, ucol = (tid % UV) * 8;  // tid < 32 UV holds a piece of the u tile
    const bool uthread = tid < 32 * UV;
    const uint4 zero = uint4{0u, 0u, 0u, 0u};
    auto load_x = [&](int64_t t0) {
        const int64_t t = t0 + xrow;
        return (t < tb1 && xcol_ok) ? *reinterpret_cast<const uint4 *>(in + t * ldin + c0 + xcol) : zero;
    };
    auto load_u = [&](int64_t t0) {
        const int64_t t = t0 + urow;
        return (uthread && t < tb1) ? *reinterpret_cast<const uint4 *>(u + t * ldu + ucol) : zero;
    };
    f32x4l acc[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[rt] = f32x4l{0.f, 0.f, 0.f, 0.f};
    uint4 rx = load_x(tb0), ru = load_u(tb0);
    int buf = 0;
    for (int64_t t0 = tb0; t0 < tb1; t0 += 32) {
        *reinterpret_cast<uint4 *>(&sx[buf][xrow][xcol]) = rx;
        if (uthread) *reinterpret_cast<uint4 *>(&su[buf][urow][ucol]) = ru;
        __syncthreads();
        if (t0 + 32 < tb1) {
            rx = load_x(t0 + 32);
            ru = load_u(t0 + 32);
        }
        uint32_t e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = sx[buf][8 * g + j][16 * wid + n];
        const uint4 xb = uint4{pack2(e[0], e[1]), pack2(e[2], e[3]), pack2(e[4], e[5]), pack2(e[6], e[7])};
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
            for (int j = 0; j < 8; ++j) e[j] = su[buf][8 * g + j][rt * 16 + n];
            const uint4 ua = uint4{pack2(e[0], e[1]), pack2(e[2], e[3]), pack2(e[4], e[5]), pack2(e[6], e[7])};
            acc[rt] = mfma(ua, xb, acc[rt]);
        }
        buf ^= 1;
    }
    if (c0 + 16 * wid >= C) return;
    float *p = part + (int64_t)blockIdx.y * Rp * C + c0 + 16 * wid + n;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int q = 0; q < 4; ++q) p[(int64_t)(rt * 16 + 4 * g + q) * C] = acc[rt][q];
}

// G[i][c] = fma(s, sum over chunks in order of part[chunk][i][c], G[i][c]) for rows i < r
__global__ __launch_bounds__(256) void lora_grad_fold_kernel(const float *__restrict__ part, int nchunks, int Rp, int r,
                                                             int64_t C, float *__restrict__ G, int64_t ldg, float s) {
    const int64_t c4 = C / 4, total = (int64_t)r * c4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / c4, c = (i % c4) * 4;
        float4 sum = float4{0.f, 0.f, 0.f, 0.f};
        for (int ch = 0; ch < nchunks; ++ch) {
            const float4 v = *reinterpret_cast<const float4 *>(part + ((int64_t)ch * Rp + row) * C + c);
            sum.x += v.x;
            sum.y += v.y;
            sum.z += v.z;
            sum.w += v.w;
        }
        float4 *gp = reinterpret_cast<float4 *>(G + row * ldg + c);
        float4 gv = *gp;
        gv.x = fmaf(s, sum.x, gv.x);
        gv.y = fmaf(s, sum.y, gv.y);
        gv.z = fmaf(s, sum.z, gv.z);
        gv.w = fmaf(s, sum.w, gv.w);
        *gp = gv;
    }
}

inline bool rank_ok(int r) { return r >= 1 && r <= 64; }
inline bool ld_ok(int64_t ld, int64_t width) { return ld >= width && ld % 8 == 0; }

}  // namespace
}  // namespace swh

using namespace swh;

extern "C" int swh_lora_down(const void *x, const void *M, void *u, int64_t T, int64_t K, int32_t r, int64_t ldx,
                             int64_t ldm, int64_t ldu, int32_t dtype, void *stream) {
    if (!x || !M || !u || T < 0 || K <= 0 || K % 32 || !rank_ok(r)) return SWH_E_ARG;
    if (dtype != SWH_BF16) return SWH_E_DTYPE;
    const int Rp = rank_pad(r);
    if (!ld_ok(ldx, K) || !ld_ok(ldm, K) || !ld_ok(ldu, Rp)) return SWH_E_ARG;
    if (!aligned16(x) || !aligned16(M) || !aligned16(u)) return SWH_E_ARG;
    if (T == 0) return SWH_OK;
    const int64_t grid = (T + 15) / 16;
    if (grid > 0x7fffffffLL) return SWH_E_ARG;
    auto xs = static_cast<const uint16_t *>(x), ms = static_cast<const uint16_t *>(M);
    auto us = static_cast<uint16_t *>(u);
    auto st = static_cast<hipStream_t>(stream);
    const dim3 gd((unsigned)grid);
    switch (Rp / 16) {
        case 1: lora_down_kernel<1><<<gd, 256, 0, st>>>(xs, ms, us, T, K, r, ldx, ldm, ldu); break;
        case 2: lora_down_kernel<2><<<gd, 256, 0, st>>>(xs, ms, us, T, K, r, ldx, ldm, ldu); break;
        case 3: lora_down_kernel<3><<<gd, 256, 0, st>>>(xs, ms, us, T, K, r, ldx, ldm, ldu); break;
        default: lora_down_kernel<4><<<gd, 256, 0, st>>>(xs, ms, us, T, K, r, ldx, ldm, ldu); break;
    }
    return launch_status();
}

extern "C" int swh_lora_up_add(const void *u, const void *M, void *y, int64_t T, int64_t C, int32_t r, int64_t ldu,
                               int64_t ldm, int64_t ldy, float scale, int32_t dtype, void *stream) {
    if (!u || !M || !y || T < 0 || C <= 0 || C % 16 || !rank_ok(r)) return SWH_E_ARG;
    if (dtype != SWH_BF16) return SWH_E_DTYPE;
    const int Rp = rank_pad(r);
    if (!ld_ok(ldu, Rp) || !ld_ok(ldm, C) || !ld_ok(ldy, C)) return SWH_E_ARG;
    if (!aligned16(u) || !aligned16(M) || !aligned16(y)) return SWH_E_ARG;
    if (T == 0) return SWH_OK;
    const int64_t gy = (T + kUpTok - 1) / kUpTok;
    if (gy > 65535) return SWH_E_ARG;
    const dim3 gd((unsigned)((C + 63) / 64), (unsigned)gy);
    auto us = static_cast<const uint16_t *>(u), ms = static_cast<const uint16_t *>(M);
    auto ys = static_cast<uint16_t *>(y);
    auto st = static_cast<hipStream_t>(stream);
    if (Rp <= 32) lora_up_add_kernel<1><<<gd, 256, 0, st>>>(us, ms, ys, T, C, Rp, ldu, ldm, ldy, scale);
    else lora_up_add_kernel<2><<<gd, 256, 0, st>>>(us, ms, ys, T, C, Rp, ldu, ldm, ldy, scale);
    return launch_status();
}

extern "C" int64_t swh_lora_grad_workspace_bytes(int64_t T, int64_t C, int32_t r) {
    if (T < 0 || C <= 0 || !rank_ok(r)) return 0;
    const int64_t nch = (T + kGradChunk - 1) / kGradChunk;
    return (nch > 0 ? nch : 1) * rank_pad(r) * C * (int64_t)sizeof(float);
}

extern "C" int swh_lora_grad(const void *u, const void *in, float *G, int64_t T, int64_t C, int32_t r, int64_t ldu,
                             int64_t ldin, int64_t ldg, float scale, int32_t dtype, void *workspace,
                             int64_t workspace_bytes, void *stream) {
    if (!u || !in || !G || !workspace || T < 0 || C <= 0 || C % 16 || !rank_ok(r)) return SWH_E_ARG;
    if (dtype != SWH_BF16) return SWH_E_DTYPE;
    const int Rp = rank_pad(r);
    if (!ld_ok(ldu, Rp) || !ld_ok(ldin, C) || ldg < C || ldg % 4) return SWH_E_ARG;
    if (!aligned16(u) || !aligned16(in) || !aligned16(G) || !aligned16(workspace)) return SWH_E_ARG;
    if (workspace_bytes < swh_lora_grad_workspace_bytes(T, C, r)) return SWH_E_ARG;
    if (T == 0) return SWH_OK;
    const int64_t nch = (T + kGradChunk - 1) / kGradChunk;
    if (nch > 65535) return SWH_E_ARG;
    const dim3 gd((unsigned)((C + 63) / 64), (unsigned)nch);
    auto us = static_cast<const uint16_t *>(u), is = static_cast<const uint16_t *>(in);
    auto part = static_cast<float *>(workspace);
    auto st = static_cast<hipStream_t>(stream);
    switch (Rp / 16) {
        case 1: lora_grad_partial_kernel<1><<<gd, 256, 0, st>>>(us, is, part, T, C, ldu, ldin); break;
        case 2: lora_grad_partial_kernel<2><<<gd, 256, 0, st>>>(us, is, part, T, C, ldu, ldin); break;
        case 3: lora_grad_partial_kernel<3><<<gd, 256, 0, st>>>(us, is, part, T, C, ldu, ldin); break;
        default: lora_grad_partial_kernel<4><<<gd, 256, 0, st>>>(us, is, part, T, C, ldu, ldin); break;
    }
    if (hipGetLastError() != hipSuccess) return SWH_E_LAUNCH;
    const int64_t total = (int64_t)r * (C / 4);
    const int64_t fg = (total + 255) / 256;
    lora_grad_fold_kernel<<<dim3((unsigned)(fg < 4096 ? fg : 4096)), 256, 0, st>>>(part, (int)nch, Rp, r, C, G, ldg,
                                                                                  scale);
    return launch_status();
}

extern "C" int64_t swh_lora_merge_tiles(int64_t N, int64_t K) {
    if (N <= 0 || K <= 0) return 0;
    return merge_tiles(N, K);
}

extern "C" int swh_lora_merge(const void *jobs, int32_t njobs, int64_t total_tiles, void *stream) {
    if (!jobs || njobs <= 0 || njobs > kMergeMaxJobs || total_tiles <= 0 || total_tiles > 0x7fffffffLL)
        return SWH_E_ARG;
    lora_merge_kernel<<<dim3((unsigned)total_tiles), 256, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const MergeJob *>(jobs), njobs);
    return launch_status();
}
