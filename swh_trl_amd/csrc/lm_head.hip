// Tile kernel of the decode step (many 16-column tiles, K <= 1024: the lm head, gate/up):
// persistent workgroups, one per CU (per M tile); the X image [64 x K] is
// staged (and normalised) once, then every wave owns whole 16-column tiles
// over the full K — all K/32 weight loads of a tile in flight at once, the
// next tile's issued as soon as the MFMAs have consumed the current one, no
// cross-wave merge.  Tile t goes to workgroup t % wgs, so every CU gets work
// even when tiles are few.  Epilogues: plain (+ bias), SiLU gate (a tile is
// 8 gate + 8 up columns), or the fused sampler.
//
// Here: lm_head_kernel (with the hand-scheduled PIPE prologue), the sampler's finalize
// (lm_sample_finalize_kernel), their launch dispatch, tile_gemm() — the way
// csrc/decode_gemm.hip reaches the plain / bias / SiLU tiles — and the
// swh_lm_head_sample* entry points.
#include <type_traits>

#include "decode_common.hpp"

namespace swh {
namespace {

// Loads the compiler does not count (the pipelined tile prologue, lm_head_kernel PIPE):
// beside an LDS-DMA in flight hipcc waits vmcnt(0) before the first use of any load it
// can see, so the weight fragments and the A-fragment LDS reads are issued from asm
// statements and retired by hand-counted waits.  A destination is valid only after the
// wait statement that names it ("+v": the compiler cannot read or copy it earlier).
__device__ __forceinline__ bf16x8 as_bf16x8(const u32x4 &v) { return __builtin_bit_cast(bf16x8, v); }
template <bool NT>
__device__ __forceinline__ void ldw_hidden(u32x4 &d, const uint16_t *p) {
    if constexpr (NT) asm volatile("global_load_dwordx4 %0, %1, off nt" : "=v"(d) : "v"(p) : "memory");
    else asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(d) : "v"(p) : "memory");
}
template <int OFF>
__device__ __forceinline__ void lds128_hidden(u32x4 &d, uint32_t base) {
    static_assert(OFF >= 0 && OFF < 65536, "ds_read offset field");
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(base), "n"(OFF) : "memory");
}
template <int N>
__device__ __forceinline__ void vm_wait() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void landed(u32x4 &d) { asm volatile("" : "+v"(d)); }  // after the wait that retires d
// at most N LDS reads younger than these four are outstanding
template <int N>
__device__ __forceinline__ void lgkm_wait(u32x4 (&a)[4]) {
    asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]) : "n"(N) : "memory");
}
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// Reductions over one 16-lane DPP row (the 16 column lanes of a C-layout row group):
// quad_perm xor 1, quad_perm xor 2, row_half_mirror, row_mirror.  Every stage pairs
// lanes symmetrically, so all 16 lanes end with bit-identical values.
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float row16_max(float v) {
    v = fmaxf(v, dpp_f<0xB1>(v));
    v = fmaxf(v, dpp_f<0x4E>(v));
    v = fmaxf(v, dpp_f<0x141>(v));
    return fmaxf(v, dpp_f<0x140>(v));
}
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_f<0xB1>(v);
    v += dpp_f<0x4E>(v);
    v += dpp_f<0x141>(v);
    return v + dpp_f<0x140>(v);
}

// KSC: K / 32 at compile time (0 = read from K): with a constant trip count the
// compiler pipelines the A-fragment LDS reads across k-steps and waits on each
// weight load in turn (vmcnt(k)), instead of one LDS round trip per MFMA
// behind a wait for the whole tile (the lm head ran 5.6 us of MFMA per tile).
// RD: weight-ring depth in k-steps (0: the whole tile, KSC).  RD = KSC / 2 holds half a
// tile per wave (the k-steps ks + RD of the same tile, then the next tile's, refill each
// register), which fits three 12-wave... waves per SIMD: 768-thread workgroups.
// SAMPLE: 0 a plain GEMM epilogue, 1 the fused sampler, 2 the fused sampler with the
// temperature division (T != 1); 3 / 4: 1 / 2 plus the log-normaliser of the processed
// scores (the drawn token's log-prob, swh_lm_head_sample_logp): per tile and row a
// 16-lane max and sum of e^(z - max), folded into one running (max, sum) per lane —
// lane rl owns row 16 (rl >> 2) + 4 g + (rl & 3) — so the state costs two registers
// PIPE: the prologue and the first tile of every wave by K chunk (below); later tiles of a
// wave and every epilogue are the PIPE = 0 code, and the arithmetic is the same MFMAs in the
// same order, so the outputs are bit-identical (tests/test_tile_pipe_gpu.py)
template <int NM, int EPI, bool BIAS, int SAMPLE, int KSC, int RD = 0, int PIPE = 0>
__global__ __launch_bounds__(RD ? 768 : 512) void lm_head_kernel(const uint16_t *__restrict__ x, const uint16_t *__restrict__ w,
                                                      int M, int N, int K, const uint16_t *__restrict__ norm_w,
                                                      float eps, const float *__restrict__ ss_in,
                                                      const uint16_t *__restrict__ bias, uint16_t *__restrict__ y,
                                                      int ldy, LmSample smp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, NT = blockDim.x, NW = NT >> 6;
    const int rl = lane & 15, kq = (lane >> 4) * 8, g = lane >> 4;
    const int nmt = (M + 63) / 64, mt = blockIdx.x % nmt, m0 = mt * 64;
    const int wgs = gridDim.x / nmt, wg = blockIdx.x / nmt;
    constexpr int KSA = KSC ? KSC : kLmMaxKS;  // register array extent
    const int ntile = (EPI == EPI_SILU) ? N / 8 : N / 16, KS = KSC ? KSC : K / 32, RS = K * 2 + 16;
    const GemmLds L = gemm_lds(1, 64, NW, K, K, NM, false);
    float *rstd_s = reinterpret_cast<float *>(lds);
    float *nw_s = reinterpret_cast<float *>(lds + L.nw_off);
    float *ssp = reinterpret_cast<float *>(lds + L.ss_off);
    unsigned char *xs = lds + L.body_off;
    const int tstep = wgs * NW;
    int t = wg + wgs * wid;  // tile t -> workgroup t % wgs
    SWH_GEMM_TRACE(0);

    static_assert(RD == 0 || (KSC != 0 && KSC % RD == 0 && 2 * RD == KSC), "RD: half of a compile-time tile");
    constexpr int KR = RD ? RD : KSA;  // weight registers per lane
    uint4 bv[KR];
    auto wrow_of = [&](int tile) -> int64_t {
        if constexpr (EPI == EPI_SILU) return (rl < 8) ? tile * 8 + rl : N + tile * 8 + rl - 8;  // gate, then up
        return (int64_t)tile * 16 + rl;
    };
    // fw 1: tile t's fragments for k-step ks at ((t KS + ks) 64 + lane) 8 (one 1 KB run per load)
    const int64_t wst = smp.fw ? 512 : 32;
    auto wbase = [&](int tile) -> const uint16_t * {
        return smp.fw ? w + ((int64_t)tile * KS * 64 + lane) * 8 : w + wrow_of(tile) * K + kq;
    };
    auto issue = [&](int tile) {
        const uint16_t *wr = wbase(tile);
#pragma unroll
        for (int ks = 0; ks < KR; ++ks)
            if (KSC || ks < KS) bv[ks] = ld_wt<EPI == EPI_SILU>(wr + ks * wst);
    };
    if (PIPE == 0 && t < ntile) issue(t);  // the weight stream first
    // RMSNorm partials and norm weights (L2), then the X image by LDS-DMA
    const int nc = K / 64;
    // folded norm: 8 lanes per row sum the row's chunk partials in registers and the
    // row statistic is in LDS by the image barrier (no LDS pass, no extra barrier)
    const bool reg_rstd = PIPE == 0 && NM == 2 && ss_in && 64 * 8 <= NT && nc <= 64;
    const bool use_ss = PIPE == 0 && NM && ss_in && 64 * nc <= 4 * NT && !reg_rstd;
    float4 ssv[4];
    float4 ss8[8];
    uint4 nwv[2];
    if (reg_rstd) {
        const int r = min(m0 + (tid >> 3), M - 1), sub = tid & 7;
        const float4 *row = reinterpret_cast<const float4 *>(ss_in + (int64_t)r * (K / 16));
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (sub + 8 * j < nc) ss8[j] = row[sub + 8 * j];
    }
    if constexpr (NM != 0) {
        if (use_ss) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int idx = min(tid + q * NT, 64 * nc - 1);
                const int r = idx / nc, c = idx - r * nc;
                ssv[q] = reinterpret_cast<const float4 *>(ss_in + (int64_t)min(m0 + r, M - 1) * (K / 16))[c];
            }
        }
        if constexpr (NM == 1) {
#pragma unroll
            for (int q = 0; q < 2; ++q) nwv[q] = reinterpret_cast<const uint4 *>(norm_w)[min(tid + q * NT, K / 8 - 1)];
        }
    }
    const int ppr = K / 8, jpl = (ppr + 63) >> 6;
    for (int r = PIPE ? 64 : wid; r < 64; r += NW) {
        const uint16_t *src = x + (int64_t)min(m0 + r, M - 1) * K;
        for (int j = 0; j < jpl; ++j) {
            const int c = lane + 64 * j;
            if (c < ppr)
                __builtin_amdgcn_global_load_lds(src + c * 8,
                                                 (__attribute__((address_space(3))) void *)(xs + r * RS + j * 1024),
                                                 16, 0, 0);
        }
    }
    if constexpr (NM != 0) {
        if (use_ss) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int idx = tid + q * NT;
                if (idx < 64 * nc) ssp[idx] = ((ssv[q].x + ssv[q].y) + ssv[q].z) + ssv[q].w;
            }
        }
#pragma unroll
        for (int q = 0; q < 2; ++q)
            if (NM == 1 && tid + q * NT < K / 8) {
                float f[8];
                unpack16<SWH_BF16>(nwv[q], f);
                reinterpret_cast<float4 *>(nw_s)[2 * (tid + q * NT)] = float4{f[0], f[1], f[2], f[3]};
                reinterpret_cast<float4 *>(nw_s)[2 * (tid + q * NT) + 1] = float4{f[4], f[5], f[6], f[7]};
            }
    }
    if constexpr (PIPE == 0) {
        SWH_GEMM_TRACE(1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // image (and this wave's first tile) landed
    }
    if (reg_rstd) {
        const int r = tid >> 3, sub = tid & 7;
        float v = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (sub + 8 * j < nc) v += ((ss8[j].x + ss8[j].y) + ss8[j].z) + ss8[j].w;
        v += __shfl_xor(v, 1);
        v += __shfl_xor(v, 2);
        v += __shfl_xor(v, 4);
        if (r < 64 && sub == 0) rstd_s[r] = rsqrtf(v / (float)K + eps);
    }
    if constexpr (PIPE == 0) {
        lds_barrier();
        SWH_GEMM_TRACE(2);
    }
    if (PIPE == 0 && NM != 0 && !reg_rstd) {
        if (tid < 64) {
            float ssum = 0.f;
            if (use_ss) {
                for (int c = 0; c < nc; ++c) ssum += ssp[tid * nc + c];
            } else {  // from the (raw) image: the whole row is here
                for (int c = 0; c < ppr; ++c) {
                    float a[8];
                    unpack16<SWH_BF16>(*reinterpret_cast<const uint4 *>(xs + tid * RS + c * 16), a);
#pragma unroll
                    for (int k = 0; k < 8; ++k) ssum = fmaf(a[k], a[k], ssum);
                }
            }
            rstd_s[tid] = rsqrtf(ssum / (float)K + eps);
        }
        lds_barrier();
    }
    // PIPE: the prologue and the wave's first tile by K chunk.  The j = 0 DMA of an image
    // row covers k-steps 0-15 and the j = 1 DMA the rest, so a wave issues: weights of
    // chunk 0, its 8 rows' j = 0 DMAs, weights of chunk 1, the j = 1 DMAs, the row
    // statistics.  vmcnt retires in order: waiting until only the instructions issued
    // after chunk 0 remain, then the barrier, proves chunk 0 of the image (every wave's
    // share) and of this wave's weights in place, and its 64 MFMAs run under the landing of
    // chunk 1.  Every wave executes the same barriers, with or without a tile.
    f32x4 acc[4];
    bool piped = false;  // the first tile's accumulators are already complete
    if constexpr (PIPE != 0) {
        static_assert(KSC > 16 && KSC <= 32 && RD == 0 && NM != 1 && SAMPLE == 0,
                      "the pipelined prologue: compile-time K of two DMA runs per row, 8 waves, no image pass");
        constexpr int KS0 = 16, KC = KSC * 32, RSC = KC * 2 + 16, PPR = KC / 8, NCC = KC / 64;
        constexpr int NSS = NM == 2 ? 2 : 0;  // row-statistic loads per lane (NCC <= 16 float4 chunks over 8 lanes)
        const bool own = __builtin_amdgcn_readfirstlane(t < ntile ? 1 : 0) != 0;
        const uint16_t *wr = wbase(own ? t : 0);
        u32x4 wv[KSC];
        auto dma = [&](int j) __attribute__((always_inline)) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int r = wid + 8 * q, c = lane + 64 * j;
                const uint16_t *src = x + (int64_t)min(m0 + r, M - 1) * KC;
                if (c < PPR)
                    __builtin_amdgcn_global_load_lds(src + c * 8,
                                                     (__attribute__((address_space(3))) void *)(xs + r * RSC + j * 1024),
                                                     16, 0, 0);
            }
        };
        if (own) static_for<0, KS0>([&](auto k) __attribute__((always_inline)) {
            ldw_hidden<EPI == EPI_SILU>(wv[decltype(k)::value], wr + decltype(k)::value * wst);
        });
        __builtin_amdgcn_sched_barrier(0);
        dma(0);
        __builtin_amdgcn_sched_barrier(0);
        if (own) static_for<KS0, KSC>([&](auto k) __attribute__((always_inline)) {
            ldw_hidden<EPI == EPI_SILU>(wv[decltype(k)::value], wr + decltype(k)::value * wst);
        });
        __builtin_amdgcn_sched_barrier(0);
        dma(1);
        __builtin_amdgcn_sched_barrier(0);
        float4 st[2];
        if constexpr (NM == 2) {
            const float4 *row =
                reinterpret_cast<const float4 *>(ss_in + (int64_t)min(m0 + (tid >> 3), M - 1) * (KC / 16));
            st[0] = row[tid & 7];
            st[1] = row[min((tid & 7) + 8, NCC - 1)];
        }
        __builtin_amdgcn_sched_barrier(0);
        SWH_GEMM_TRACE(1);
        // still in flight after chunk 0: chunk 1's weights (a wave with a tile), 8 DMAs, the statistics
        if (own) vm_wait<KSC - KS0 + 8 + NSS>();
        else vm_wait<8 + NSS>();
        lds_barrier();
        SWH_GEMM_TRACE(7);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        // A fragments one k-step ahead, as the later tiles; rows 16 i of the image from two
        // bases (the ds_read offset field is 16 bits)
        const uint32_t xa0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) unsigned char *)(
            xs + rl * RSC + kq * 2);
        const uint32_t xa2 = xa0 + 32 * RSC;
        u32x4 a[2][4];
        auto read_a = [&](auto k, u32x4(&d)[4]) __attribute__((always_inline)) {
            constexpr int ks = decltype(k)::value;
            lds128_hidden<ks * 64>(d[0], xa0);
            lds128_hidden<16 * RSC + ks * 64>(d[1], xa0);
            lds128_hidden<ks * 64>(d[2], xa2);
            lds128_hidden<16 * RSC + ks * 64>(d[3], xa2);
        };
        auto mma_chunk = [&](auto k0, auto k1) __attribute__((always_inline)) {
            constexpr int K0 = decltype(k0)::value, K1 = decltype(k1)::value;
            static_for<K0, K1>([&](auto k) __attribute__((always_inline)) { landed(wv[decltype(k)::value]); });
            read_a(k0, a[K0 & 1]);
            static_for<K0, K1>([&](auto k) __attribute__((always_inline)) {
                constexpr int ks = decltype(k)::value;
                if constexpr (ks + 1 < K1) read_a(std::integral_constant<int, ks + 1>{}, a[(ks + 1) & 1]);
                lgkm_wait<(ks + 1 < K1) ? 4 : 0>(a[ks & 1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(a[ks & 1][i]), as_bf16x8(wv[ks]), acc[i],
                                                                    0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            });
        };
        if (own) mma_chunk(std::integral_constant<int, 0>{}, std::integral_constant<int, KS0>{});
        vm_wait<0>();  // chunk 1: everything this wave issued
        lds_barrier();
        SWH_GEMM_TRACE(2);
        if (own) mma_chunk(std::integral_constant<int, KS0>{}, std::integral_constant<int, KSC>{});
        piped = own;
        if constexpr (NM == 2) {  // the row statistic, needed by the epilogue only
            const int r = tid >> 3, sub = tid & 7;
            float v = 0.f;
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (sub + 8 * j < NCC) v += ((st[j].x + st[j].y) + st[j].z) + st[j].w;
            v += __shfl_xor(v, 1);
            v += __shfl_xor(v, 2);
            v += __shfl_xor(v, 4);
            if (sub == 0) rstd_s[r] = rsqrtf(v / (float)KC + eps);
            lds_barrier();
        }
    }
    SWH_GEMM_TRACE(3);
    float rsr[4][4];  // folded RMSNorm (NM 2): the row scale of each accumulator row
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) rsr[i][e] = (NM == 2) ? rstd_s[i * 16 + 4 * g + e] : 1.f;
    if constexpr (NM == 1) {
        int r = tid / ppr, c = tid - r * ppr;
        const int rstep = NT / ppr, cstep = NT - rstep * ppr;
        while (r < 64) {
            uint4 *pv = reinterpret_cast<uint4 *>(xs + r * RS + c * 16);
            const float4 *wv = reinterpret_cast<const float4 *>(nw_s) + 2 * c;
            *pv = norm_frag(*pv, wv[0], wv[1], rstd_s[r]);
            r += rstep;
            c += cstep;
            if (c >= ppr) {
                c -= ppr;
                ++r;
            }
        }
        lds_barrier();
    }
    // sampler state: per lane the best (key, column) of its 16 rows 16 i + 4 g + e
    constexpr bool TDIV = SAMPLE == 2 || SAMPLE == 4, LOGP = SAMPLE >= 3;
    float bk[4][4];
    int32_t bi[4][4];
    uint32_t k0 = 0, k1 = 0, clo = 0, chi = 0;
    bool suppress = false;
    float temp = 1.f;
    float lm_run = kNegInf, ls_run = 0.f;  // LOGP: the owned row's running (max, sum e^(z - max))
    if constexpr (SAMPLE) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                bk[i][e] = kNegInf;
                bi[i][e] = 0x7fffffff;
            }
        const int32_t step = *smp.step;
        const uint64_t seed = smp.rng[0], ctr = smp.rng[1] + (uint64_t)step;
        k0 = (uint32_t)seed;
        k1 = (uint32_t)(seed >> 32);
        clo = (uint32_t)ctr;
        chi = (uint32_t)(ctr >> 32);
        suppress = step < smp.p.min_new_tokens;
        temp = (!smp.p.greedy && smp.p.temperature != 1.0f) ? smp.p.temperature : 1.f;
    }
    for (; t < ntile; t += tstep) {
        // (PIPE: the first tile is accumulated; its successor's weights are issued whole,
        // below, once no hidden load is in flight)
        const bool mma = !(PIPE != 0 && piped);
        piped = false;
        if (mma) {
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const unsigned char *xrow = xs + rl * RS + kq * 2;
        // ring refill: k-step ks's weight register takes the next tile's fragment as
        // soon as its MFMA has read it, so a wave always has KS loads in flight
        const bool ring = mma && KSC != 0 && t + tstep < ntile;
        const uint16_t *wnext = wbase(ring ? t + tstep : t);
        const uint16_t *wcur = wbase(t);
        if (!mma) {
            // accumulated by the pipelined prologue
        } else if constexpr (KSC != 0) {
            // A fragments double-buffered one k-step ahead (2 and 3 ahead measured no faster
            // for gate/up: 11.24 / 11.38-11.42 against 11.15-11.21 us, profiles/r5_gu_apf_ab.log);
            // the scheduling barrier keeps the compiler from hoisting every read
            constexpr int APF = 1, AR = APF + 1;
            uint4 a[AR][4];
#pragma unroll
            for (int p = 0; p < APF; ++p)
#pragma unroll
                for (int i = 0; i < 4; ++i) a[p][i] = *reinterpret_cast<const uint4 *>(xrow + i * 16 * RS + p * 64);
#pragma unroll
            for (int ks = 0; ks < KSC; ++ks) {
                if (ks + APF < KSC) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        a[(ks + APF) % AR][i] = *reinterpret_cast<const uint4 *>(xrow + i * 16 * RS + (ks + APF) * 64);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(a[ks % AR][i]), as_bf16x8(bv[ks % KR]),
                                                                    acc[i], 0, 0, 0);
                if constexpr (RD != 0) {  // half-tile ring: this tile's second half, then the next tile's first
                    if (ks + KR < KSC) bv[ks % KR] = ld_wt<EPI == EPI_SILU>(wcur + (ks + KR) * wst);
                    else if (ring) bv[ks % KR] = ld_wt<EPI == EPI_SILU>(wnext + (ks + KR - KSC) * wst);
                } else if (ring) {
                    bv[ks] = ld_wt<EPI == EPI_SILU>(wnext + ks * wst);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll
            for (int ks = 0; ks < KSA; ++ks) {
                if (ks < KS) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const uint4 a = *reinterpret_cast<const uint4 *>(xrow + i * 16 * RS + ks * 64);
                        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(a), as_bf16x8(bv[ks]), acc[i], 0, 0, 0);
                    }
                }
            }
        }
        if (!ring && t + tstep < ntile) issue(t + tstep);
        SWH_GEMM_TRACE(4);
        if constexpr (SAMPLE) {
            const int col = t * 16 + rl;
            // EOS suppression as an added -inf (x + 0 = x), not a branch per element; the
            // temperature division only in the SAMPLE == 2 instantiation (T != 1): as a select,
            // the IEEE division ran on every element at T = 1 too
            float mask_add = 0.f;
            if (suppress) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < smp.p.n_eos && col == smp.p.eos_ids[e]) mask_add = kNegInf;
            }
            float own_m = kNegInf, own_s = 0.f;  // LOGP: this tile's (max, sum) of the lane's owned row
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                U4 rw{0u, 0u, 0u, 0u};
                if (!smp.p.greedy) rw = philox4x32_10(U4{(uint32_t)col, (uint32_t)((m0 >> 2) + 4 * i + g), clo, chi}, k0, k1);
                const uint32_t wd[4] = {rw.x, rw.y, rw.z, rw.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float z = round_bf16(acc[i][e] * rsr[i][e]);  // the bf16 logit
                    if constexpr (TDIV) z = z / temp;
                    if constexpr (LOGP) {  // the processed score z + mask over the row's 16 tile columns
                        const float zp = z + mask_add;
                        const float mx = row16_max(zp);
                        const float sx = row16_sum(fast_exp(fmaxf(zp - mx, -1.0e4f)));
                        const bool own = rl == 4 * i + e;
                        own_m = own ? mx : own_m;
                        own_s = own ? sx : own_s;
                    }
                    float key = smp.p.greedy ? z : z + gumbel_from_bits(wd[e]);
                    key += mask_add;
                    // branch-free: a lane's columns grow with t, so the index tie-break only
                    // ever fires against the initial (-inf, INT_MAX) entry
                    const bool better = (key > bk[i][e]) | ((key == bk[i][e]) & (col < bi[i][e]));
                    bk[i][e] = better ? key : bk[i][e];
                    bi[i][e] = better ? col : bi[i][e];
                }
            }
            if constexpr (LOGP) {  // fold the tile into the owned row's running state
                if (own_m != kNegInf) {
                    const float nm = fmaxf(lm_run, own_m);
                    ls_run = (lm_run == kNegInf ? 0.f : ls_run * fast_exp(lm_run - nm)) + own_s * fast_exp(own_m - nm);
                    lm_run = nm;
                }
            }
        } else if constexpr (EPI == EPI_SILU) {
            // lanes rl < 8 hold gate column t*8+rl, lanes rl+8 the matching up column.
            // Both lanes of a pair can form y = bf16(silu(gate)) * up of their column:
            // the gate lanes take rows 0-31 of the tile, the up lanes rows 32-63, into
            // the wave's 1 KB LDS tile [64 rows][8 columns]; then lane r stores row r's
            // 8 columns (16 contiguous bytes in the fragment order and row-major alike)
            // as one 16-B store instead of 16 scattered 2-B stores.
            uint16_t *yt = reinterpret_cast<uint16_t *>(lds + L.total) + wid * 512;
            const bool gl = rl < 8;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = round_bf16(acc[i][e] * rsr[i][e]);
                    const float u = __shfl_xor(v, 8, kWave);
                    if (gl == (i < 2)) {
                        const float gt = gl ? v : u, up = gl ? u : v;
                        yt[(i * 16 + 4 * g + e) * 8 + (rl & 7)] = f32_to_bf16_bits(round_bf16(gt / (1.f + expf(-gt))) * up);
                    }
                }
            const uint4 yr = *reinterpret_cast<const uint4 *>(yt + lane * 8);
            const int row = m0 + lane, col = t * 8;  // yf: ((row/16 * N/32 + col/32) 64 + row%16 + 16 (col/8 % 4)) 8
            if (row < M) {
                const int64_t at = smp.yf ? (((int64_t)(row >> 4) * (N >> 5) + (col >> 5)) * 64 +
                                             ((col >> 3) & 3) * 16 + (row & 15)) * 8
                                          : (int64_t)row * ldy + col;
                *reinterpret_cast<uint4 *>(y + at) = yr;
            }
        } else {
            // C layout: lane holds rows 16 i + 4 g + e of column rl.  Through the wave's
            // 2 KB LDS tile [64 rows][16 columns], lane r stores row r's 16 columns as
            // two 16-B pieces (not 16 scattered 2-B stores).
            const float bz = BIAS ? bf16_bits_to_f32(bias[t * 16 + rl]) : 0.f;
            uint16_t *yt = reinterpret_cast<uint16_t *>(lds + L.total) + wid * 1024;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    yt[(i * 16 + 4 * g + e) * 16 + rl] = f32_to_bf16_bits(acc[i][e] * rsr[i][e] + bz);
            const uint4 y0 = *reinterpret_cast<const uint4 *>(yt + lane * 16);
            const uint4 y1 = *reinterpret_cast<const uint4 *>(yt + lane * 16 + 8);
            if (m0 + lane < M) {
                uint4 *dst = reinterpret_cast<uint4 *>(y + (int64_t)(m0 + lane) * ldy + t * 16);
                dst[0] = y0;
                dst[1] = y1;
            }
        }
    }
    SWH_GEMM_TRACE(5);
    if constexpr (SAMPLE) {
        // best over the 16 column lanes per wave, then over the workgroup's waves
        // through LDS (the X image is free once every wave is past its tiles):
        // one partial per (row, workgroup) for the finalize
        LmPart *wpart = reinterpret_cast<LmPart *>(xs);  // [NW][64]
        float2 *wsoft = reinterpret_cast<float2 *>(xs + NW * 64 * sizeof(LmPart));  // LOGP: [NW][64]
        __syncthreads();
        if constexpr (LOGP) wsoft[wid * 64 + 16 * (rl >> 2) + 4 * g + (rl & 3)] = float2{lm_run, ls_run};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float k = bk[i][e];
                int32_t c = bi[i][e];
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) {
                    const float k2 = __shfl_xor(k, o, kWave);
                    const int32_t c2 = __shfl_xor(c, o, kWave);
                    if (k2 > k || (k2 == k && (uint32_t)c2 < (uint32_t)c)) {
                        k = k2;
                        c = c2;
                    }
                }
                if (rl == 0) wpart[wid * 64 + i * 16 + 4 * g + e] = LmPart{k, c};
            }
        __syncthreads();
        if (tid < 64 && m0 + tid < M) {
            LmPart bpart = wpart[tid];
            for (int q = 1; q < NW; ++q) {
                const LmPart o = wpart[q * 64 + tid];
                if (o.key > bpart.key || (o.key == bpart.key && (uint32_t)o.idx < (uint32_t)bpart.idx)) bpart = o;
            }
            smp.part[(int64_t)(m0 + tid) * smp.pstride + wg] = bpart;
            if constexpr (LOGP) {
                SoftState st = soft_init();
                for (int q = 0; q < NW; ++q) st = soft_merge(st, SoftState{wsoft[q * 64 + tid].x, wsoft[q * 64 + tid].y, 0.f});
                smp.lpart[(int64_t)(m0 + tid) * smp.pstride + wg] = float2{st.m, st.s1};
            }
        }
    }
    SWH_GEMM_TRACE(6);
}

// Merge the per-wave partials of a row; EOS / pad bookkeeping as
// swh_sample_step's finalize (csrc/sampler.hip).
// LOGP (lpart, out_logp non-null): the row's (max, sum) partials are merged too and
// out_logp[b, step] = z - max - log(sum) for the drawn column's processed score z,
// recovered as key + log(-log(u)) of the same Philox draw (the key itself when greedy):
// within an fp32 rounding of the key (~1e-6 at |z| ~ 10) of the score the logits path sees.
__global__ __launch_bounds__(256) void lm_sample_finalize_kernel(const LmPart *__restrict__ part, int P,
                                                                 swh_sample_params p, const int32_t *__restrict__ step_p,
                                                                 int32_t *__restrict__ finished,
                                                                 int64_t *__restrict__ out_tokens, int64_t out_ld,
                                                                 int64_t *__restrict__ cur_tokens, int V, LmNext nx,
                                                                 const float2 *__restrict__ lpart = nullptr,
                                                                 float *__restrict__ out_logp = nullptr,
                                                                 const uint64_t *__restrict__ rng = nullptr) {
    __shared__ float kk[4];
    __shared__ int32_t ii[4];
    __shared__ float sm[4], ssum[4];
    __shared__ int64_t tok_s;
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const bool logp = lpart && out_logp;
    float k = kNegInf;
    int32_t c = 0x7fffffff;
    SoftState st = soft_init();
    for (int q = tid; q < P; q += 256) {
        const LmPart v = part[b * P + q];
        if (v.key > k || (v.key == k && (uint32_t)v.idx < (uint32_t)c)) {
            k = v.key;
            c = v.idx;
        }
        if (logp) st = soft_merge(st, SoftState{lpart[b * P + q].x, lpart[b * P + q].y, 0.f});
    }
    if (logp) {
        st = wave_soft(st);
        if (lane == 0) {
            sm[wid] = st.m;
            ssum[wid] = st.s1;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float k2 = __shfl_xor(k, o, kWave);
        const int32_t c2 = __shfl_xor(c, o, kWave);
        if (k2 > k || (k2 == k && (uint32_t)c2 < (uint32_t)c)) {
            k = k2;
            c = c2;
        }
    }
    if (lane == 0) {
        kk[wid] = k;
        ii[wid] = c;
    }
    __syncthreads();
    if (tid == 0) {
        for (int q = 1; q < 4; ++q)
            if (kk[q] > k || (kk[q] == k && (uint32_t)ii[q] < (uint32_t)c)) {
                k = kk[q];
                c = ii[q];
            }
        if (c < 0 || c >= V) c = 0;  // fully masked row (cannot happen with min_tokens_to_keep=1)
        const int32_t step = *step_p;
        if (logp) {
            SoftState r = soft_init();
            for (int q = 0; q < 4; ++q) r = soft_merge(r, SoftState{sm[q], ssum[q], 0.f});
            float z = k;
            if (!p.greedy) {
                const uint64_t seed = rng[0], ctr = rng[1] + (uint64_t)step;
                const U4 w4 = philox4x32_10(U4{(uint32_t)c, (uint32_t)(b >> 2), (uint32_t)ctr, (uint32_t)(ctr >> 32)},
                                            (uint32_t)seed, (uint32_t)(seed >> 32));
                const uint32_t q = (uint32_t)(b & 3);
                const uint32_t bits = q == 0 ? w4.x : q == 1 ? w4.y : q == 2 ? w4.z : w4.w;
                z = k - gumbel_from_bits(bits);
            }
            out_logp[b * out_ld + step] = (z - r.m) - fast_log(r.s1);
        }
        int64_t tok = c;
        if (p.pad_token_id >= 0 && finished[b] != 0) tok = p.pad_token_id;
        bool is_eos = false;
        for (int e = 0; e < p.n_eos && e < 4; ++e) is_eos |= (tok == p.eos_ids[e]);
        if (is_eos) finished[b] = 1;
        out_tokens[b * out_ld + step] = tok;
        if (cur_tokens) cur_tokens[b] = tok;
        tok_s = tok;
    }
    if (!nx.embed) return;
    __syncthreads();
    // the next step's input row: embedding of the drawn token + its RMSNorm partials
    const int64_t id = tok_s;
    const int nch = nx.H / 16;
    for (int ch = tid; ch < nch; ch += 256) {
        const uint4 *src = reinterpret_cast<const uint4 *>(nx.embed + id * nx.H) + 2 * ch;
        const uint4 lo = src[0], hi = src[1];
        uint4 *dst = reinterpret_cast<uint4 *>(nx.x + b * nx.H) + 2 * ch;
        dst[0] = lo;
        dst[1] = hi;
        if (nx.ss) {
            float a[8], e[8];
            unpack16<SWH_BF16>(lo, a);
            unpack16<SWH_BF16>(hi, e);
            float ss = 0.f;
#pragma unroll
            for (int q = 0; q < 8; ++q) ss = fmaf(a[q], a[q], ss);
#pragma unroll
            for (int q = 0; q < 8; ++q) ss = fmaf(e[q], e[q], ss);
            nx.ss[b * nch + ch] = ss;
        }
    }
    if (tid == 0) {  // every row has read *step before its ticket: the last one advances it
        const int t = __hip_atomic_fetch_add(nx.ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (t == nx.M - 1) {
            __hip_atomic_store(nx.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(nx.step, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <int NM, int EPI, bool BIAS, int SAMPLE, int KSC, int RD = 0, int PIPE = 0>
int launch_lm_ks(dim3 grid, size_t lds, hipStream_t s, const uint16_t *X, const uint16_t *W, int M, int N, int K,
                 const uint16_t *NWt, float eps, const float *ss_in, const uint16_t *Bs, uint16_t *Y, int ldy,
                 const LmSample &smp) {
    if (!lds_opt_in<&lm_head_kernel<NM, EPI, BIAS, SAMPLE, KSC, RD, PIPE>>()) return SWH_E_LAUNCH;  // > 64 KB LDS
    lm_head_kernel<NM, EPI, BIAS, SAMPLE, KSC, RD, PIPE><<<grid, RD ? 768 : 512, lds, s>>>(X, W, M, N, K, NWt, eps, ss_in,
                                                                                        Bs, Y, ldy, smp);
    return launch_status();
}

// the fused sampler at K = 896 with the half-tile weight ring and 12 waves per workgroup
// (three per SIMD): 58.2-58.8 against 60.3-60.4 us per launch, bench +0.6 % (launch policy
// lm_ring14 = 0: off; read per call)
inline bool lm_ring14() { return launch_policy().lm_ring14 != 0; }

// the pipelined prologue (lm_head_kernel PIPE): the first tile's MFMAs of k-steps 0-15 under
// the landing of the rest of the X image (launch policy tile_pipe, read per call).  It has
// no pass over the image, so it takes plain X or the folded norm with the row statistics
// given; the fused sampler keeps the load-all prologue (its log-prob variants sit at
// 251-253 VGPRs and the K = 896 sampler runs 12 waves, where a wave's image share differs).
template <int NM, int SAMPLE>
inline bool tile_pipe(const float *ss_in) {
    return SAMPLE == 0 && (NM == 0 || (NM == 2 && ss_in)) && launch_policy().tile_pipe != 0;
}

// compile-time k-step counts for the model widths in use (Qwen2.5-0.5B: H = 896)
template <int NM, int EPI, bool BIAS, int SAMPLE>
int launch_lm(dim3 grid, size_t lds, hipStream_t s, const uint16_t *X, const uint16_t *W, int M, int N, int K,
              const uint16_t *NWt, float eps, const float *ss_in, const uint16_t *Bs, uint16_t *Y, int ldy,
              const LmSample &smp) {
    if constexpr (SAMPLE == 1 || SAMPLE == 3) {  // the division instantiation when the rows are sampled at T != 1
        if (!smp.p.greedy && smp.p.temperature != 1.0f)
            return launch_lm<NM, EPI, BIAS, SAMPLE + 1>(grid, lds, s, X, W, M, N, K, NWt, eps, ss_in, Bs, Y, ldy, smp);
    }
    switch (K / 32) {
    case 28:
        if ((SAMPLE == 1 || SAMPLE == 2) && lm_ring14())  // (the log-prob variants spill at 768 threads)
            return launch_lm_ks<NM, EPI, BIAS, SAMPLE, 28, 14>(grid, lds, s, X, W, M, N, K, NWt, eps, ss_in, Bs, Y, ldy,
                                                               smp);
        if constexpr (SAMPLE == 0 && NM != 1) {
            if (tile_pipe<NM, SAMPLE>(ss_in))
                return launch_lm_ks<NM, EPI, BIAS, SAMPLE, 28, 0, 1>(grid, lds, s, X, W, M, N, K, NWt, eps, ss_in, Bs, Y,
                                                                    ldy, smp);
        }
        return launch_lm_ks<NM, EPI, BIAS, SAMPLE, 28>(grid, lds, s, X, W, M, N, K, NWt, eps, ss_in, Bs, Y, ldy, smp);
    case 32:
        if constexpr (SAMPLE == 0 && NM != 1) {
            if (tile_pipe<NM, SAMPLE>(ss_in))
                return launch_lm_ks<NM, EPI, BIAS, SAMPLE, 32, 0, 1>(grid, lds, s, X, W, M, N, K, NWt, eps, ss_in, Bs, Y,
                                                                    ldy, smp);
        }
        return launch_lm_ks<NM, EPI, BIAS, SAMPLE, 32>(grid, lds, s, X, W, M, N, K, NWt, eps, ss_in, Bs, Y, ldy, smp);
    default: return launch_lm_ks<NM, EPI, BIAS, SAMPLE, 0>(grid, lds, s, X, W, M, N, K, NWt, eps, ss_in, Bs, Y, ldy, smp);
    }
}


// the tile kernel for plain / bias / SiLU epilogues
template <int EPI, bool BIAS>
int launch_tiles(int nm, dim3 grid, size_t lds, hipStream_t s, const uint16_t *X, const uint16_t *W, int M, int N,
                 int K, const uint16_t *NWt, float eps, const float *ss_in, const uint16_t *Bs, uint16_t *Y, int ldy,
                 int fw, int yf = 0) {
    LmSample none{};
    none.fw = fw;
    none.yf = yf;
    if (nm == 1) return launch_lm<1, EPI, BIAS, false>(grid, lds, s, X, W, M, N, K, NWt, eps, ss_in, Bs, Y, ldy, none);
    if (nm == 2) return launch_lm<2, EPI, BIAS, false>(grid, lds, s, X, W, M, N, K, nullptr, eps, ss_in, Bs, Y, ldy, none);
    return launch_lm<0, EPI, BIAS, false>(grid, lds, s, X, W, M, N, K, nullptr, eps, nullptr, Bs, Y, ldy, none);
}

}  // namespace

int tile_gemm(int epi, int nm, dim3 grid, size_t lds, hipStream_t s, const uint16_t *X, const uint16_t *W, int M, int N,
              int K, const uint16_t *NWt, float eps, const float *ss_in, const uint16_t *Bs, uint16_t *Y, int ldy,
              int fw, int yf) {
    if (epi == EPI_SILU) return launch_tiles<EPI_SILU, false>(nm, grid, lds, s, X, W, M, N, K, NWt, eps, ss_in, Bs, Y, ldy, fw, yf);
    if (Bs) return launch_tiles<EPI_PLAIN, true>(nm, grid, lds, s, X, W, M, N, K, NWt, eps, ss_in, Bs, Y, ldy, fw);
    return launch_tiles<EPI_PLAIN, false>(nm, grid, lds, s, X, W, M, N, K, NWt, eps, ss_in, Bs, Y, ldy, fw);
}

}  // namespace swh

using namespace swh;

// [partials (M x per x 8 LmPart) | 256 B: the finalize ticket (zero at allocation) |
//  the log-prob variant's (max, sum) partials, M x per x 8 float2]
static int64_t lm_part_bytes(int64_t M, int64_t V = 0) {
    const int64_t nmt = (M + 63) / 64, per = cu_count() / nmt > 0 ? cu_count() / nmt : 1;
    const int64_t wide = V / 256 + 1;  // the wide sampler's partials per row (K > 1024)
    return (M * (per * 8 > wide ? per * 8 : wide) * (int64_t)sizeof(LmPart) + 255) / 256 * 256;
}

extern "C" int64_t swh_lm_head_sample_workspace_bytes(int64_t M, int64_t V, int64_t K) {
    (void)K;
    return 2 * lm_part_bytes(M, V) + 256;  // sizeof(float2) == sizeof(LmPart)
}

static int lm_head_sample_impl(const void *x, const void *w, int64_t M, int64_t V, int64_t K, const void *norm_w,
                               float eps, const float *ss_in, const swh_sample_params *params, const uint64_t *rng,
                               const int32_t *step, int32_t *finished, int64_t *out_tokens, int64_t out_ld,
                               int64_t *cur_tokens, void *workspace, int64_t workspace_bytes, LmNext nx, void *stream,
                               int fw = 0, float *out_logp = nullptr) {
    if (fw && (norm_w || K % 128)) return SWH_E_ARG;  // fragment order: folded weight (ss_in row scale) only
    if (out_logp && fw && K > 32 * kLmMaxKS) return SWH_E_ARG;  // log-probs: the tile kernel (K <= 1024) only
    // K > 1024 (Llama-3-8B): a fragment-order (= wide_pack order) weight through wide_gemm's
    // 256-row tiles with the sampler epilogue, M <= 64, V % 256 == 0
    const bool wide = fw && K > 32 * kLmMaxKS;
    if (!x || !w || !params || !rng || !step || !finished || !out_tokens || !workspace || M <= 0 || V <= 0 ||
        K <= 0 || K % 64 || (K > 32 * kLmMaxKS && !wide) || V % 16 || V >= ((int64_t)1 << 31) || M > (1 << 20))
        return SWH_E_ARG;
    const swh_sample_params p = *params;
    const bool filtered = !p.greedy && ((p.top_k > 0 && p.top_k < V) || p.top_p < 1.0f || p.min_p > 0.f);
    if (filtered || p.repetition_penalty != 1.0f || p.n_eos < 0 || p.n_eos > 4 || !(p.temperature > 0.f))
        return SWH_E_ARG;  // the caller takes logits + swh_sample_step
    if (workspace_bytes < swh_lm_head_sample_workspace_bytes(M, V, K)) return SWH_E_ARG;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w)) & 15) return SWH_E_ARG;
    if ((norm_w && (reinterpret_cast<uintptr_t>(norm_w) & 15)) || (ss_in && (reinterpret_cast<uintptr_t>(ss_in) & 15)))
        return SWH_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (wide) {
        int pstride = 0;
        LmPart *part = static_cast<LmPart *>(workspace);
        const int rc = wide_lm_sample(x, w, M, V, K, eps, ss_in, p, rng, step, part, &pstride, s);
        if (rc == 1) return SWH_E_ARG;  // not a wide shape: logits + swh_sample_step
        if (rc != SWH_OK) return rc;
        lm_sample_finalize_kernel<<<dim3((unsigned)M), 256, 0, s>>>(part, pstride, p, step, finished, out_tokens,
                                                                   out_ld, cur_tokens, (int)V, nx);
        return launch_status();
    }
    const int64_t nmt = (M + 63) / 64, per = cu_count() / nmt > 0 ? cu_count() / nmt : 1;
    const int nm = norm_w ? 1 : (ss_in ? 2 : 0);
    const GemmLds L = gemm_lds(1, 64, 8, (int)K, (int)K, nm, false);
    const dim3 grid((unsigned)(per * nmt));
    LmSample smp{p, rng, step, static_cast<LmPart *>(workspace), (int)per, fw};  // one partial per (row, workgroup)
    if (out_logp)
        smp.lpart = reinterpret_cast<float2 *>(static_cast<char *>(workspace) + lm_part_bytes(M, V) + 256);
    const auto *X = static_cast<const uint16_t *>(x);
    const auto *W = static_cast<const uint16_t *>(w);
    const auto *NWt = static_cast<const uint16_t *>(norm_w);
    const size_t lds = (size_t)L.total;
    const int iM = (int)M, iV = (int)V, iK = (int)K;
    int rc;
    if (out_logp)
        rc = nm == 1   ? launch_lm<1, EPI_PLAIN, false, 3>(grid, lds, s, X, W, iM, iV, iK, NWt, eps, ss_in, nullptr, nullptr, 0, smp)
             : nm == 2 ? launch_lm<2, EPI_PLAIN, false, 3>(grid, lds, s, X, W, iM, iV, iK, nullptr, eps, ss_in, nullptr, nullptr, 0, smp)
                       : launch_lm<0, EPI_PLAIN, false, 3>(grid, lds, s, X, W, iM, iV, iK, nullptr, eps, nullptr, nullptr, nullptr, 0, smp);
    else
        rc = nm == 1   ? launch_lm<1, EPI_PLAIN, false, 1>(grid, lds, s, X, W, iM, iV, iK, NWt, eps, ss_in, nullptr, nullptr, 0, smp)
             : nm == 2 ? launch_lm<2, EPI_PLAIN, false, 1>(grid, lds, s, X, W, iM, iV, iK, nullptr, eps, ss_in, nullptr, nullptr, 0, smp)
                       : launch_lm<0, EPI_PLAIN, false, 1>(grid, lds, s, X, W, iM, iV, iK, nullptr, eps, nullptr, nullptr, nullptr, 0, smp);
    if (rc != SWH_OK) return rc;
    lm_sample_finalize_kernel<<<dim3((unsigned)M), 256, 0, s>>>(smp.part, smp.pstride, p, step, finished, out_tokens,
                                                               out_ld, cur_tokens, (int)V, nx, smp.lpart, out_logp, rng);
    return launch_status();
}

extern "C" int swh_lm_head_sample(const void *x, const void *w, int64_t M, int64_t V, int64_t K, const void *norm_w,
                                  float eps, const float *ss_in, const swh_sample_params *params, const uint64_t *rng,
                                  const int32_t *step, int32_t *finished, int64_t *out_tokens, int64_t out_ld,
                                  int64_t *cur_tokens, void *workspace, int64_t workspace_bytes, void *stream) {
    return lm_head_sample_impl(x, w, M, V, K, norm_w, eps, ss_in, params, rng, step, finished, out_tokens, out_ld,
                               cur_tokens, workspace, workspace_bytes, LmNext{}, stream);
}

static int lm_head_sample_step_impl(const void *x, const void *w, int64_t M, int64_t V, int64_t K,
                                    const void *norm_w, float eps, const float *ss_in,
                                    const swh_sample_params *params, const uint64_t *rng, int32_t *step,
                                    int32_t *finished, int64_t *out_tokens, int64_t out_ld, int64_t *cur_tokens,
                                    const void *embed, void *x_next, float *ss_next, void *workspace,
                                    int64_t workspace_bytes, void *stream, int fw) {
    if (!embed || !x_next || !cur_tokens || K % 16) return SWH_E_ARG;
    if ((reinterpret_cast<uintptr_t>(embed) | reinterpret_cast<uintptr_t>(x_next)) & 15) return SWH_E_ARG;
    if (workspace_bytes < swh_lm_head_sample_workspace_bytes(M, V, K)) return SWH_E_ARG;
    LmNext nx{static_cast<const uint16_t *>(embed), static_cast<uint16_t *>(x_next), ss_next, step,
              reinterpret_cast<int32_t *>(static_cast<char *>(workspace) + lm_part_bytes(M, V)), (int)K, (int)M};
    return lm_head_sample_impl(x, w, M, V, K, norm_w, eps, ss_in, params, rng, step, finished, out_tokens, out_ld,
                               cur_tokens, workspace, workspace_bytes, nx, stream, fw);
}

extern "C" int swh_lm_head_sample_step(const void *x, const void *w, int64_t M, int64_t V, int64_t K,
                                       const void *norm_w, float eps, const float *ss_in,
                                       const swh_sample_params *params, const uint64_t *rng, int32_t *step,
                                       int32_t *finished, int64_t *out_tokens, int64_t out_ld, int64_t *cur_tokens,
                                       const void *embed, void *x_next, float *ss_next, void *workspace,
                                       int64_t workspace_bytes, void *stream) {
    return lm_head_sample_step_impl(x, w, M, V, K, norm_w, eps, ss_in, params, rng, step, finished, out_tokens,
                                    out_ld, cur_tokens, embed, x_next, ss_next, workspace, workspace_bytes, stream, 0);
}

extern "C" int swh_lm_head_sample_fragw(const void *x, const void *w, int64_t M, int64_t V, int64_t K, float eps,
                                        const float *ss_in, const swh_sample_params *params, const uint64_t *rng,
                                        const int32_t *step, int32_t *finished, int64_t *out_tokens, int64_t out_ld,
                                        int64_t *cur_tokens, void *workspace, int64_t workspace_bytes, void *stream) {
    return lm_head_sample_impl(x, w, M, V, K, nullptr, eps, ss_in, params, rng, step, finished, out_tokens, out_ld,
                               cur_tokens, workspace, workspace_bytes, LmNext{}, stream, 1);
}

extern "C" int swh_lm_head_sample_step_fragw(const void *x, const void *w, int64_t M, int64_t V, int64_t K,
                                             float eps, const float *ss_in, const swh_sample_params *params,
                                             const uint64_t *rng, int32_t *step, int32_t *finished,
                                             int64_t *out_tokens, int64_t out_ld, int64_t *cur_tokens,
                                             const void *embed, void *x_next, float *ss_next, void *workspace,
                                             int64_t workspace_bytes, void *stream) {
    return lm_head_sample_step_impl(x, w, M, V, K, nullptr, eps, ss_in, params, rng, step, finished, out_tokens,
                                    out_ld, cur_tokens, embed, x_next, ss_next, workspace, workspace_bytes, stream, 1);
}

// The fused sampler with the drawn token's log-prob under the processed distribution
// (SAMPLE 3 / 4 of lm_head_kernel): one entry for both weight orders, with or without
// the next step's input (embed null: none, the step counter is not advanced).
extern "C" int swh_lm_head_sample_logp(const void *x, const void *w, int64_t M, int64_t V, int64_t K,
                                       const void *norm_w, float eps, const float *ss_in, int32_t frag_weights,
                                       const swh_sample_params *params, const uint64_t *rng, int32_t *step,
                                       int32_t *finished, int64_t *out_tokens, int64_t out_ld, int64_t *cur_tokens,
                                       float *out_logp, const void *embed, void *x_next, float *ss_next,
                                       void *workspace, int64_t workspace_bytes, void *stream) {
    if (!out_logp || (frag_weights & ~1) || K > 32 * kLmMaxKS) return SWH_E_ARG;
    LmNext nx{};
    if (embed) {
        if (!x_next || !cur_tokens || K % 16) return SWH_E_ARG;
        if ((reinterpret_cast<uintptr_t>(embed) | reinterpret_cast<uintptr_t>(x_next)) & 15) return SWH_E_ARG;
        if (workspace_bytes < swh_lm_head_sample_workspace_bytes(M, V, K)) return SWH_E_ARG;
        nx = LmNext{static_cast<const uint16_t *>(embed), static_cast<uint16_t *>(x_next), ss_next, step,
                    reinterpret_cast<int32_t *>(static_cast<char *>(workspace) + lm_part_bytes(M, V)), (int)K, (int)M};
    }
    return lm_head_sample_impl(x, w, M, V, K, norm_w, eps, ss_in, params, rng, step, finished, out_tokens, out_ld,
                               cur_tokens, workspace, workspace_bytes, nx, stream, frag_weights, out_logp);
}
