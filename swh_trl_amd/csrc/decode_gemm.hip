// Decode-step projections of the rollout engine (batch <= 64 rows per tile):
//
//  * swh_decode_gemm — weight-streaming "skinny" GEMM  Y[M,N] = X[M,K] W[N,K]^T
//    on MFMA v_mfma_f32_16x16x32_bf16, with the decoder's neighbours fused:
//      prologue  RMSNorm of X (Qwen2RMSNorm rounding points)      [qkv, gate_up, lm head]
//      epilogue  + bias                                           [qkv]
//                residual: s = bf16(s + bf16(acc)) in place       [o_proj, down_proj]
//                          + per-row sums of squares of the new s (the next RMSNorm)
//                SiLU gate: y = bf16(bf16(silu(bf16 g)) * bf16 u) [gate_up]
//    A workgroup owns all 64 rows x NB = 16*CB output columns of one K slice;
//    its NW waves (4/8/16) split the slice's k-steps and each wave issues ALL
//    the weight/X loads of a round of U k-steps at once (one HBM round trip
//    per round, tail clamped rather than looped), so a launch costs about one
//    weight-load latency plus the merge.  W (the only HBM stream) is read
//    exactly once, with nontemporal loads; X and the norm weight are L2-hot.
//    The RMSNorm statistic comes precomputed from the kernel that produced X
//    (ss_in: fp32 partial sums over 16-column chunks), so no workgroup re-reads
//    whole X rows in a prologue.  Replaces the hipBLASLt M=64 GEMMs (measured
//    0.6 TB/s) plus the separate RMSNorm / SiLU / residual launches.
//
// Here: the split-K kernel (decode_gemm_kernel), its register-streamed sibling for
// short K (xstream_gemm_kernel), the cost model and the launch dispatch.  Many
// 16-column tiles at K <= 1024 (gate/up, the lm head) go to the tile kernel of
// csrc/lm_head.hip, K >= the policy's wide_kmin to csrc/wide_gemm.hip.
#include "decode_common.hpp"

namespace swh {
namespace {

// Tile = MR (16 * MS) rows x NB (16 * CB) output columns x one K slice.
// A workgroup stages its X slice [MR rows x Kr] into LDS ONCE — every wave
// whole rows, lanes along the row (full-line 16-B loads), RMSNorm applied on
// the way in — then covers one column block, or several when the grid is
// smaller than the column blocks (the lm head loops, prefetching the next
// block's weights before merging the current one).  The NW waves split the
// slice's k-steps; each issues all weight loads of a round of U k-steps at
// once (fragment order) and takes its A fragments from the LDS image.  Waves
// merge through a fixed-order LDS tree.  Tiles are numbered so the M tiles of
// one column block land on one XCD (dispatch is round-robin over the 8 XCDs):
// their shared weight rows are fetched from HBM once and re-read from that
// XCD's L2.  S > 1: write-through (sc1) fp32 slabs, an agent-scope ticket, the
// last arriver sums the S slabs in fixed order (deterministic, placement-
// independent — MI355X_MICROARCH.md §Workgroup dispatch) and runs the epilogue.

// KL: a K-class tag (0: K <= 1024, 1: longer) that only separates the rocprof
// names of otherwise identical instantiations (o_proj K 896 vs down_proj K 4864)
template <int CB, int MS, int NM, int EPI, bool BIAS, int MAXT, int KL = 0>
__global__ __launch_bounds__(MAXT) void decode_gemm_kernel(
    const uint16_t *__restrict__ x, const uint16_t *__restrict__ w, int M, int N, int K,
    const uint16_t *__restrict__ norm_w, float eps, const float *__restrict__ ss_in,
    const uint16_t *__restrict__ bias, uint16_t *__restrict__ res, float *__restrict__ ss_out,
    uint16_t *__restrict__ y, int ldy, float *__restrict__ slabs, int *__restrict__ counters, int persist,
    int wn, int fw) {
    // a wave computes NB = 16 CB columns; the WN column groups of NW / WN waves each
    // make a tile of NBT = WN NB columns (the waves of a group split K)
    constexpr int NB = 16 * CB, MR = 16 * MS, LDR = MR + 4;  // merge slots column-major: b128 parks
    // k-steps whose loads are issued together (the weight-load round depth); 8 / 16 / 24:
    // no gain or slower, 16 spills ("Deeper weight rounds")
    constexpr int kU = 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, NT = blockDim.x, NW = NT >> 6;
    const int WN = wn, NBT = NB * WN, WK = NW / WN, cg = wid / WK, kw = wid - cg * WK;
    const int G8 = (EPI == EPI_SILU) ? CB * WN : NBT / 8;  // 8-column output groups per row
    const int S = gridDim.z, sidx = blockIdx.z;
    const int ncb = (EPI == EPI_SILU) ? N / (NBT / 2) : N / NBT;
    const int nmt = (M + MR - 1) / MR;
    // ---- tile of this workgroup
    int cb_first, cb_step, mt;
    if (persist) {  // gridDim.x % nmt == 0
        mt = blockIdx.x % nmt;
        cb_first = blockIdx.x / nmt;
        cb_step = gridDim.x / nmt;
        if (cb_first >= ncb) return;
    } else {        // the nmt M tiles of a column block on one XCD
        const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
        cb_first = (j / nmt) * 8 + xcd;
        mt = j % nmt;
        cb_step = ncb;
        if (cb_first >= ncb) return;
    }
    const int m0 = mt * MR;
    const int KS = K / 32, kb0 = (int)((int64_t)KS * sidx / S), kb1 = (int)((int64_t)KS * (sidx + 1) / S);
    const int Kr = (kb1 - kb0) * 32, k0 = kb0 * 32, RS = Kr * 2 + 16;
    const GemmLds L = gemm_lds(CB * WN, MR, NW, (KS + S - 1) / S * 32, K, NM, persist != 0, WN);
    float *rstd_s = reinterpret_cast<float *>(lds);
    int *flag_s = reinterpret_cast<int *>(lds + 256);
    float *nw_s = reinterpret_cast<float *>(lds + L.nw_off);
    unsigned char *xs = lds + L.body_off;
    float *ssp = reinterpret_cast<float *>(lds + L.ss_off);
    float *part = reinterpret_cast<float *>(lds + L.slots_off);
    const int rl = lane & 15, kq = (lane >> 4) * 8;
    SWH_GEMM_TRACE(0);

    // ---- (a) this wave's weights for the first column block (HBM, the long pole: first in the queue)
    const int ksw0 = kb0 + (kb1 - kb0) * kw / WK, ksw1 = kb0 + (kb1 - kb0) * (kw + 1) / WK;
    const uint16_t *wrow[CB];
    auto set_rows = [&](int n0) {
#pragma unroll
        for (int j = 0; j < CB; ++j) {
            int n;
            if constexpr (EPI == EPI_SILU) {
                const int c = (cg * CB + j) * 8 + (rl & 7);
                n = (rl < 8) ? n0 + c : N + n0 + c;  // gate rows, then the matching up rows
            } else {
                n = n0 + (cg * CB + j) * 16 + rl;
            }
            // fw: the swh_frag_pack layout — 16-row group g, k-step ks, lane at ((g KS + ks) 64 + lane) 8
            // (SiLU: a 16-lane group is 8 gate + the 8 matching up rows = pack group (first gate row) / 8)
            const int64_t grp = (EPI == EPI_SILU) ? (n0 + (cg * CB + j) * 8) >> 3 : (n0 + (cg * CB + j) * 16) >> 4;
            wrow[j] = fw ? w + (grp * KS * 64 + lane) * 8 : w + (int64_t)n * K + kq;
        }
    };
    const int wstep = fw ? 512 : 32;  // elements between a lane's consecutive k-steps
    uint4 bv[kU][CB];
    auto issue = [&](int ks) {  // only this wave's k-steps: no duplicate loads
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            if (ks + u < ksw1) {
#pragma unroll
                for (int j = 0; j < CB; ++j)  // plain loads: the line's other half is the next k-step's load
                    bv[u][j] = ld_w(wrow[j] + (ks + u) * wstep);
            }
        }
    };
    auto col0 = [&](int cbk) { return cbk * (EPI == EPI_SILU ? NBT / 2 : NBT); };
    set_rows(col0(cb_first));
    issue(ksw0);
    // ---- (b) RMSNorm partial sums and the norm-weight slice (L2)
    const int nc = K / 64;
    // folded norm, one column block: the row statistic only scales the epilogue;
    // 8 lanes per row sum the row's chunk partials in registers (no LDS pass)
    const bool late_rstd = NM == 2 && !persist && ss_in && MR * 8 <= NT && nc <= 64;
    const bool use_ss = NM && ss_in && MR * nc <= 4 * NT && !late_rstd;
    float4 ssv[4];
    float4 ss8[8];
    uint4 nwv[2];
    if (late_rstd) {
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
                const int idx = min(tid + q * NT, MR * nc - 1);
                const int r = idx / nc, c = idx - r * nc;
                ssv[q] = reinterpret_cast<const float4 *>(ss_in + (int64_t)min(m0 + r, M - 1) * (K / 16))[c];
            }
        }
        if constexpr (NM == 1) {
#pragma unroll
            for (int q = 0; q < 2; ++q)
                nwv[q] = reinterpret_cast<const uint4 *>(norm_w + k0)[min(tid + q * NT, Kr / 8 - 1)];
        }
    }
    // epilogue operands of a single-block workgroup (L2): <= 2 per thread in every geometry
    const int ncol0 = col0(cb_first);
    uint4 pre_res[2], pre_bias[2];
    if constexpr (EPI == EPI_RESIDUAL || BIAS) {
        if (!persist) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int idx = min(tid + q * NT, MR * G8 - 1);
                const int r = idx / G8, gc = ncol0 + (idx - r * G8) * 8;
                if constexpr (EPI == EPI_RESIDUAL)
                    pre_res[q] = *reinterpret_cast<const uint4 *>(res + (int64_t)min(m0 + r, M - 1) * ldy + gc);
                if constexpr (BIAS) pre_bias[q] = *reinterpret_cast<const uint4 *>(bias + gc);
            }
        }
    }
    // ---- (c) X slice -> LDS image by LDS-DMA (no registers): each wave whole rows
    // wid, wid+NW, ...; one instruction = 64 lanes x 16 B = 1 KB of a row
    const int ppr = Kr / 8, jpl = (ppr + 63) >> 6;  // 16-B pieces per row, instructions per row
    for (int r = wid; r < MR; r += NW) {
        const uint16_t *src = x + (int64_t)min(m0 + r, M - 1) * K + k0;
        for (int j = 0; j < jpl; ++j) {
            const int c = lane + 64 * j;
            if (c < ppr)
                __builtin_amdgcn_global_load_lds(src + c * 8,
                                                 (__attribute__((address_space(3))) void *)(xs + r * RS + j * 1024),
                                                 16, 0, 0);
        }
    }
    // everything this workgroup streams is in flight; the image is usable once all of it landed
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    lds_barrier();
    SWH_GEMM_TRACE(1);

    // ---- (d) row statistic and norm weights into LDS
    if (late_rstd) {  // read by the epilogue only, behind the merge barriers
        const int r = tid >> 3, sub = tid & 7;
        float v = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (sub + 8 * j < nc) v += ((ss8[j].x + ss8[j].y) + ss8[j].z) + ss8[j].w;
        v += __shfl_xor(v, 1);
        v += __shfl_xor(v, 2);
        v += __shfl_xor(v, 4);
        if (r < MR && sub == 0) rstd_s[r] = rsqrtf(v / (float)K + eps);
    } else if constexpr (NM != 0) {
        if (use_ss) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int idx = tid + q * NT;
                if (idx < MR * nc) ssp[idx] = ((ssv[q].x + ssv[q].y) + ssv[q].z) + ssv[q].w;
            }
        }
#pragma unroll
        for (int q = 0; q < 2; ++q)
            if (NM == 1 && tid + q * NT < Kr / 8) {
                float f[8];
                unpack16<SWH_BF16>(nwv[q], f);
                reinterpret_cast<float4 *>(nw_s)[2 * (tid + q * NT)] = float4{f[0], f[1], f[2], f[3]};
                reinterpret_cast<float4 *>(nw_s)[2 * (tid + q * NT) + 1] = float4{f[4], f[5], f[6], f[7]};
            }
        lds_barrier();
        if (use_ss) {
            if (tid < MR) {
                float ssum = 0.f;
                for (int c = 0; c < nc; ++c) ssum += ssp[tid * nc + c];
                rstd_s[tid] = rsqrtf(ssum / (float)K + eps);
            }
        } else {
            // whole-row pass over X in global memory, one wave per row (coalesced)
            const int nv = K / 8;
            for (int r = wid; r < MR; r += NW) {
                const uint4 *xr = reinterpret_cast<const uint4 *>(x + (int64_t)min(m0 + r, M - 1) * K);
                float ss = 0.f;
                for (int v = lane; v < nv; v += 64) {
                    float a[8];
                    unpack16<SWH_BF16>(xr[v], a);
#pragma unroll
                    for (int k = 0; k < 8; ++k) ss = fmaf(a[k], a[k], ss);
                }
                ss = wave_sum(ss);
                if (lane == 0) rstd_s[r] = rsqrtf(ss / (float)K + eps);
            }
        }
        lds_barrier();
    }
    SWH_GEMM_TRACE(2);

    // ---- (e) the X image normalised in place
    if constexpr (NM == 1) {
        int r = tid / ppr, c = tid - r * ppr;
        const int rstep = NT / ppr, cstep = NT - rstep * ppr;
        for (; r < MR;) {
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
    SWH_GEMM_TRACE(3);

    // ---- (f) column blocks
    auto slot = [&](int s, int r, int c) -> float & { return part[(s * NBT + c) * LDR + r]; };
    const int F = WK;  // the merged slot
    for (int cbk = cb_first; cbk < ncb; cbk += cb_step) {
        const int n0 = col0(cbk);
        f32x4 acc[MS][CB];
#pragma unroll
        for (int i = 0; i < MS; ++i)
#pragma unroll
            for (int j = 0; j < CB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        const unsigned char *xrow = xs + rl * RS + kq * 2;
        for (int ks = ksw0; ks < ksw1; ks += kU) {
            if (ks != ksw0) issue(ks);
            const unsigned char *xk = xrow + (ks - kb0) * 64;
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                if (ks + u >= ksw1) break;
                uint4 a[MS];
#pragma unroll
                for (int i = 0; i < MS; ++i) a[i] = *reinterpret_cast<const uint4 *>(xk + i * 16 * RS + u * 64);
#pragma unroll
                for (int i = 0; i < MS; ++i)
#pragma unroll
                    for (int j = 0; j < CB; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(a[i]), as_bf16x8(bv[u][j]),
                                                                            acc[i][j], 0, 0, 0);
            }
        }
        // the next column block's first weight round overlaps this block's merge
        if (cbk + cb_step < ncb) {
            set_rows(col0(cbk + cb_step));
            issue(ksw0);
        }
        SWH_GEMM_TRACE(4);

        // ---- merge the NW waves: fixed-order tree through the LDS slots -> slot F
        // (C layout: lane holds rows 16 i + 4 g .. +3 of column 16 j + rl -> one 16-B store each)
        if (!persist) lds_barrier();  // the slots reuse the X image
        auto park = [&](int s) {
#pragma unroll
            for (int i = 0; i < MS; ++i)
#pragma unroll
                for (int j = 0; j < CB; ++j)
                    *reinterpret_cast<f32x4 *>(&slot(s, i * 16 + (lane >> 4) * 4, (cg * CB + j) * 16 + rl)) = acc[i][j];
        };
        for (int h = WK >> 1; h >= 1; h >>= 1) {
            if (kw >= h && kw < 2 * h) park(kw - h);
            lds_barrier();
            if (kw < h) {
#pragma unroll
                for (int i = 0; i < MS; ++i)
#pragma unroll
                    for (int j = 0; j < CB; ++j)
                        acc[i][j] += *reinterpret_cast<const f32x4 *>(
                            &slot(kw, i * 16 + (lane >> 4) * 4, (cg * CB + j) * 16 + rl));
            }
            lds_barrier();
        }
        if (kw == 0) park(F);
        lds_barrier();
        SWH_GEMM_TRACE(5);

        // ---- cross-workgroup split-K: publish, ticket, last arriver reduces
        if (S > 1) {
            const int blk = mt * ncb + cbk;
            float *my = slabs + ((int64_t)blk * S + sidx) * (MR * NBT);
            for (int idx = tid; idx < MR * NBT; idx += NT)
                __hip_atomic_store(my + idx, slot(F, idx / NBT, idx % NBT), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) {
                const int t = __hip_atomic_fetch_add(counters + blk, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                flag_s[0] = (t == S - 1);
            }
            __syncthreads();
            if (!flag_s[0]) return;  // S > 1 never loops over column blocks
            const float *base = slabs + (int64_t)blk * S * (MR * NBT);
            for (int idx = tid; idx < MR * NBT; idx += NT) {
                float v = 0.f;
                for (int q = 0; q < S; ++q)
                    v += __hip_atomic_load(base + (int64_t)q * MR * NBT + idx, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                slot(F, idx / NBT, idx % NBT) = v;
            }
            if (tid == 0) __hip_atomic_store(counters + blk, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
        }

        // ---- epilogue, 8 output columns (16 B) per thread
        if constexpr (EPI == EPI_SILU) {
            for (int idx = tid; idx < MR * G8; idx += NT) {
                const int r = idx / G8, jb = idx - r * G8;
                const int gr = m0 + r;
                if (gr >= M) continue;
                float o[8];
                const float sc = (NM == 2) ? rstd_s[r] : 1.f;  // folded RMSNorm: y = rstd * (x W'^T)
#pragma unroll
                for (int cc = 0; cc < 8; ++cc) {
                    const float g = round_bf16(slot(F, r, jb * 16 + cc) * sc);
                    const float u = round_bf16(slot(F, r, jb * 16 + 8 + cc) * sc);
                    o[cc] = round_bf16(g / (1.f + expf(-g))) * u;
                }
                *reinterpret_cast<uint4 *>(y + (int64_t)gr * ldy + n0 + jb * 8) = pack8(o);
            }
        } else {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int idx = tid + q * NT;
                if (idx >= MR * G8) break;
                const int r = idx / G8, c8 = (idx - r * G8) * 8;
                const int gr = m0 + r, gc = n0 + c8;
                if (gr >= M) continue;
                float v[8];
                const float sc = (NM == 2) ? rstd_s[r] : 1.f;  // folded RMSNorm: y = rstd * (x W'^T)
#pragma unroll
                for (int cc = 0; cc < 8; ++cc) v[cc] = slot(F, r, c8 + cc) * sc;
                if constexpr (BIAS) {
                    float b[8];
                    unpack16<SWH_BF16>(persist ? *reinterpret_cast<const uint4 *>(bias + gc) : pre_bias[q], b);
#pragma unroll
                    for (int cc = 0; cc < 8; ++cc) v[cc] += b[cc];
                }
                if constexpr (EPI == EPI_RESIDUAL) {
                    uint4 *sp = reinterpret_cast<uint4 *>(res + (int64_t)gr * ldy + gc);
                    float sres[8];
                    unpack16<SWH_BF16>(persist ? *sp : pre_res[q], sres);
#pragma unroll
                    for (int cc = 0; cc < 8; ++cc) {
                        sres[cc] = round_bf16(sres[cc] + round_bf16(v[cc]));
                        slot(F, r, c8 + cc) = sres[cc];
                    }
                    *sp = pack8(sres);
                } else {
                    *reinterpret_cast<uint4 *>(y + (int64_t)gr * ldy + gc) = pack8(v);
                }
            }
            if constexpr (EPI == EPI_RESIDUAL) {
                if (ss_out) {  // partial sums of squares of the new rows, per 16-column chunk
                    __syncthreads();
                    for (int idx = tid; idx < MR * CB * WN; idx += NT) {
                        const int r = idx / (CB * WN), j = idx - r * (CB * WN);
                        if (m0 + r >= M) continue;
                        float ss = 0.f;
#pragma unroll
                        for (int cc = 0; cc < 16; ++cc) ss = fmaf(slot(F, r, j * 16 + cc), slot(F, r, j * 16 + cc), ss);
                        ss_out[(int64_t)(m0 + r) * (N / 16) + n0 / 16 + j] = ss;
                    }
                }
            }
        }
        if (persist) __syncthreads();  // slot 0 is rewritten by the next block
    }
    SWH_GEMM_TRACE(6);
}

// ---------------------------------------------------------------------------
// Register-streamed short-K projection (decode qkv and o_proj at K <= 2048:
// 16 MS-row x 16-column tiles over the full K, no K split): decode_gemm_kernel
// <1, MS, NM, EPI, BIAS> with the X slice read as MFMA A fragments straight
// into registers beside the weight fragments.  A wave's A operand is X[MR rows,
// its own k-steps], which no other wave reads, so the LDS image — and its
// landing wait (vmcnt(0)) before the first MFMA — goes: every k-step of the
// wave is issued at once (KW of them) and the MFMAs consume them in arrival
// order.  Same k-step split, wave order, merge tree, row statistic and
// epilogues as decode_gemm_kernel, so the result is bit-identical.  At long K
// (down_proj, K 4864) the fragment-order X loads (64 B of a row per lane group,
// twice the lines of the image's whole-row loads) cost more than the landing
// wait saves (11.4 -> 12.4 us), so it serves K <= 2048 only.
// ---------------------------------------------------------------------------
template <int KW, int MS, int NM, int EPI, bool BIAS, int KL>
__global__ __launch_bounds__(512) void xstream_gemm_kernel(const uint16_t *__restrict__ x,
                                                           const uint16_t *__restrict__ w, int M, int N, int K,
                                                           float eps, const float *__restrict__ ss_in,
                                                           const uint16_t *__restrict__ bias,
                                                           uint16_t *__restrict__ res, float *__restrict__ ss_out,
                                                           uint16_t *__restrict__ y, int ldy, int fw, int xf) {
    static_assert(EPI != EPI_SILU && NM != 1, "plain / residual epilogues, folded or no norm");
    constexpr int NW = 8, NT = 512, MR = 16 * MS, NB = 16, LDR = MR + 4, G8 = NB / 8, F = NW;
    __shared__ __attribute__((aligned(16))) float part[(NW + 1) * NB * LDR];
    __shared__ float rstd_s[MR];
    const int tid = threadIdx.x, lane = tid & 63, kw = tid >> 6;
    const int ncb = N / NB, nmt = (M + MR - 1) / MR;
    const int xcd = blockIdx.x & 7, jj = blockIdx.x >> 3;  // the nmt M tiles of a column block on one XCD
    const int cbk = (jj / nmt) * 8 + xcd, mt = jj % nmt;
    if (cbk >= ncb) return;
    const int m0 = mt * MR, n0 = cbk * NB;
    const int KS = K / 32, ksw0 = KS * kw / NW, ksw1 = KS * (kw + 1) / NW;
    const int rl = lane & 15, kq = (lane >> 4) * 8;
    SWH_GEMM_TRACE(0);
    // epilogue operands and the row statistic's partials (oldest in the queue)
    uint4 pre_ep;
    {
        const int idx = min(tid, MR * G8 - 1);
        const int r = idx / G8, gc = n0 + (idx - r * G8) * 8;
        if constexpr (EPI == EPI_RESIDUAL)
            pre_ep = *reinterpret_cast<const uint4 *>(res + (int64_t)min(m0 + r, M - 1) * ldy + gc);
        else if constexpr (BIAS)
            pre_ep = *reinterpret_cast<const uint4 *>(bias + gc);
    }
    const int nc = K / 64;
    float4 ss8[8];
    if constexpr (NM == 2) {
        const int r = min(m0 + (tid >> 3), M - 1), sub = tid & 7;
        const float4 *row = reinterpret_cast<const float4 *>(ss_in + (int64_t)r * (K / 16));
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (sub + 8 * j < nc) ss8[j] = row[sub + 8 * j];
    }
    // fw: the swh_frag_pack layout (one contiguous 1 KB per wave and k-step)
    const uint16_t *wr = fw ? w + ((int64_t)(n0 >> 4) * KS * 64 + lane) * 8 : w + (int64_t)(n0 + rl) * K + kq;
    const int wstep = fw ? 512 : 32;
    // xf: X itself in the fragment order (16-row groups; written so by the SiLU tile
    // epilogue, M % 16 == 0): one contiguous 1 KB run per A-fragment load as well
    const uint16_t *xr[MS];
#pragma unroll
    for (int i = 0; i < MS; ++i)
        xr[i] = xf ? x + ((int64_t)((m0 >> 4) + i) * KS * 64 + lane) * 8
                   : x + (int64_t)min(m0 + i * 16 + rl, M - 1) * K + kq;
    const int xstep = xf ? 512 : 32;
    uint4 xa[KW][MS], bv[KW];
#pragma unroll
    for (int u = 0; u < KW; ++u) {
        const int ks = min(ksw0 + u, ksw1 - 1);  // past the wave's range: a repeated, unused load (no branch)
        bv[u] = ld_w(wr + ks * wstep);
#pragma unroll
        for (int i = 0; i < MS; ++i) xa[u][i] = *reinterpret_cast<const uint4 *>(xr[i] + ks * xstep);
    }
    SWH_GEMM_TRACE(1);
    if constexpr (NM == 2) {  // read by the epilogue only, behind the merge barriers
        const int r = tid >> 3, sub = tid & 7;
        float v = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (sub + 8 * j < nc) v += ((ss8[j].x + ss8[j].y) + ss8[j].z) + ss8[j].w;
        v += __shfl_xor(v, 1);
        v += __shfl_xor(v, 2);
        v += __shfl_xor(v, 4);
        if (r < MR && sub == 0) rstd_s[r] = rsqrtf(v / (float)K + eps);
    }
    f32x4 acc[MS];
#pragma unroll
    for (int i = 0; i < MS; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < KW; ++u)
        if (ksw0 + u < ksw1) {
#pragma unroll
            for (int i = 0; i < MS; ++i)
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(xa[u][i]), as_bf16x8(bv[u]), acc[i], 0, 0, 0);
        }
    SWH_GEMM_TRACE(4);
    // merge the 8 waves: decode_gemm_kernel's fixed-order tree -> slot F
    auto slot = [&](int s, int r, int c) -> float & { return part[(s * NB + c) * LDR + r]; };
    auto park = [&](int s) {
#pragma unroll
        for (int i = 0; i < MS; ++i) *reinterpret_cast<f32x4 *>(&slot(s, i * 16 + (lane >> 4) * 4, rl)) = acc[i];
    };
    for (int h = NW >> 1; h >= 1; h >>= 1) {
        if (kw >= h && kw < 2 * h) park(kw - h);
        lds_barrier();
        if (kw < h) {
#pragma unroll
            for (int i = 0; i < MS; ++i) acc[i] += *reinterpret_cast<const f32x4 *>(&slot(kw, i * 16 + (lane >> 4) * 4, rl));
        }
        lds_barrier();
    }
    if (kw == 0) park(F);
    lds_barrier();
    SWH_GEMM_TRACE(5);
    // epilogue, 8 output columns (16 B) per thread
    if (tid < MR * G8) {
        const int r = tid / G8, c8 = (tid - r * G8) * 8;
        const int gr = m0 + r, gc = n0 + c8;
        if (gr < M) {
            float v[8];
            const float sc = (NM == 2) ? rstd_s[r] : 1.f;  // folded RMSNorm: y = rstd * (x W'^T)
#pragma unroll
            for (int cc = 0; cc < 8; ++cc) v[cc] = slot(F, r, c8 + cc) * sc;
            if constexpr (EPI == EPI_RESIDUAL) {
                float sres[8];
                unpack16<SWH_BF16>(pre_ep, sres);
#pragma unroll
                for (int cc = 0; cc < 8; ++cc) {
                    sres[cc] = round_bf16(sres[cc] + round_bf16(v[cc]));
                    slot(F, r, c8 + cc) = sres[cc];
                }
                *reinterpret_cast<uint4 *>(res + (int64_t)gr * ldy + gc) = pack8(sres);
            } else {
                if constexpr (BIAS) {
                    float b[8];
                    unpack16<SWH_BF16>(pre_ep, b);
#pragma unroll
                    for (int cc = 0; cc < 8; ++cc) v[cc] += b[cc];
                }
                *reinterpret_cast<uint4 *>(y + (int64_t)gr * ldy + gc) = pack8(v);
            }
        }
    }
    if constexpr (EPI == EPI_RESIDUAL) {
        if (ss_out) {  // partial sums of squares of the new rows over this 16-column chunk
            __syncthreads();
            if (tid < MR && m0 + tid < M) {
                float ss = 0.f;
#pragma unroll
                for (int cc = 0; cc < 16; ++cc) ss = fmaf(slot(F, tid, cc), slot(F, tid, cc), ss);
                ss_out[(int64_t)(m0 + tid) * (N / 16) + n0 / 16] = ss;
            }
        }
    }
    SWH_GEMM_TRACE(6);
}

// ---- GEMM launch configuration -------------------------------------------
// The smallest K routed to csrc/wide_gemm.hip and whether that path is on come from
// the launch policy (swh_set_launch_policy; the DecodeEngine reads the same policy to
// choose its packed projections), read per call on the host (at graph capture).

struct GemmCfg {
    int ms, cb, nw, s, gx;  // 16-row blocks, 16-col blocks (tile), waves, K split, grid.x
    bool persist;
    int wn = 1;             // column groups: a wave computes cb / wn column blocks over K / (nw / wn)
    int fw = 0;             // weights in the swh_frag_pack layout
    int xf = 0;             // X (the SiLU activation) in the same fragment order (xstream only)
};

// 8 waves in every geometry: more k-steps in flight per CU (down 14.9 -> 11.5 us,
// qkv 7.0 -> 6.3 us against 4 waves for 16- and 32-row tiles; tools/bench_decode.py --ku)
inline int gemm_waves(int) { return 8; }

// Modelled launch time (us) of one geometry — measured shape of the cost on
// MI355X (tools/gemm_probe.py, tools/bench_decode.py --sweep): a fixed
// ~3 us, the bytes one CU pulls through its load path at ~60 GB/s (weights in
// fragment order count twice), ~1 us per 10k elements of in-LDS RMSNorm,
// +9 us for a cross-workgroup split, +3 us per extra wave of workgroups.
double gemm_cost(const GemmCfg &c, int64_t M, int64_t wcols, int64_t K, int nm) {
    const int64_t MR = 16 * c.ms, KS = K / 32, ncu = cu_count();
    const int64_t krmax = (KS + c.s - 1) / c.s * 32;
    const GemmLds L = gemm_lds(c.cb, (int)MR, c.nw, (int)krmax, (int)K, nm, c.persist, c.wn);
    if (L.total > 160 * 1024) return 1e30;
    if (c.cb % c.wn || c.nw % c.wn || MR * c.cb * 2 > 2 * 64 * c.nw) return 1e30;  // epilogue: <= 2 groups / thread
    const int64_t ncb = wcols / (16 * c.cb), nmt = (M + MR - 1) / MR;
    const int64_t xbytes = MR * krmax * 2, wbytes = 2 * 16 * c.cb * krmax * 2;
    if (c.persist) {
        const int64_t wgs = c.gx, per = (ncb + wgs / nmt - 1) / (wgs / nmt);
        return 3.0 + (xbytes + per * wbytes) / 60e3;
    }
    const int64_t wgs = 8 * nmt * ((ncb + 7) / 8) * c.s;
    int64_t res = (160 * 1024) / L.total;
    res = res < 1 ? 1 : (res > 2 ? 2 : res);
    const int64_t per_cu = (wgs + ncu - 1) / ncu, waves = (wgs + ncu * res - 1) / (ncu * res);
    const double norm_us = nm == 1 ? (double)(MR * krmax) / 10e3 : 0.0;  // in-LDS RMSNorm pass
    return 3.0 + per_cu * ((xbytes + wbytes) / 60e3 + norm_us) + (c.s > 1 ? 9.0 : 0.0) + (waves - 1) * 3.0;
}

GemmCfg pick_cfg(int64_t M, int64_t wcols, int64_t K, bool silu, int nm) {
    const int64_t KS = K / 32, align = silu ? 2 : 1, ncu = cu_count();
    GemmCfg best{4, 4, 8, 1, 0, false};
    double best_cost = 1e31;
    for (int ms : {1, 2, 4})
        for (int cb : {1, 2, 4}) {
            if (wcols % (16 * cb * align)) continue;
            for (int sp = 1; sp <= 8; ++sp) {
                if (sp > KS) break;
                GemmCfg c{ms, cb, gemm_waves(ms), sp, 0, false};
                const double t = gemm_cost(c, M, wcols, K, nm);
                if (t < best_cost) {
                    best_cost = t;
                    best = c;
                }
            }
        }
    // persistent: all 64 rows, 32-column blocks, grid = the CUs, weights streamed once
    const int64_t nmt64 = (M + 63) / 64;
    if (wcols % (32 * align) == 0 && ncu / nmt64 >= 1) {
        GemmCfg c{4, 2, 8, 1, (int)((ncu / nmt64) * nmt64), true};
        if (c.gx > wcols / 32 * nmt64) c.gx = (int)(wcols / 32 * nmt64);
        if (gemm_cost(c, M, wcols, K, nm) < best_cost) best = c;
    }
    const swh_launch_policy pol = launch_policy();
    if (pol.gemm_ms) {  // geometry override of the launch policy (tests / A/B)
        const int a = pol.gemm_ms, b = pol.gemm_cb, d = pol.gemm_s, pz = pol.gemm_persist, wn = pol.gemm_wn;
        if ((a == 1 || a == 2 || a == 4) && (b == 1 || b == 2 || b == 4) && d >= 1 && d <= KS && d <= 8 &&
            wcols % (16 * b * align) == 0 && !(pz && d != 1) && (wn == 1 || wn == 2 || wn == 4)) {
            const int64_t nmt = (M + 16 * a - 1) / (16 * a);
            GemmCfg c{a, b, gemm_waves(a), d, 0, pz != 0, wn};
            if (c.persist) {
                const int64_t per = ncu / nmt > 0 ? ncu / nmt : 1, ncb = wcols / (16 * b);
                c.gx = (int)((per < ncb ? per : ncb) * nmt);
            }
            if (gemm_cost(c, M, wcols, K, nm) < 1e29) best = c;
        }
    }
    if (!best.persist) best.gx = (int)(8 * ((M + 16 * best.ms - 1) / (16 * best.ms)) * ((wcols / (16 * best.cb) + 7) / 8));
    // one column block per wave (column groups split the waves, each group splits K):
    // a 4x smaller LDS merge; gate/up 14.7 -> 12.3 us (tools/bench_decode.py --ku)
    if (!pol.gemm_ms && !best.persist && best.cb > 1 && best.nw % best.cb == 0 &&
        gemm_cost(GemmCfg{best.ms, best.cb, best.nw, best.s, best.gx, false, best.cb}, M, wcols, K, nm) < 1e29)
        best.wn = best.cb;
    if (pol.gemm_nw) {  // policy override: waves per workgroup (16: cb == 1 only)
        const int v = pol.gemm_nw;
        if ((v == 4 || v == 8 || (v == 16 && best.cb == best.wn)) &&
            gemm_cost(GemmCfg{best.ms, best.cb, v, best.s, best.gx, best.persist, best.wn}, M, wcols, K, nm) < 1e29)
            best.nw = v;
    }
    return best;
}

int64_t slab_bytes(const GemmCfg &c, int64_t M, int64_t wcols) {
    if (c.s == 1) return 0;
    const int64_t MR = 16 * c.ms, nmt = (M + MR - 1) / MR;
    return nmt * wcols * c.s * MR * (int64_t)sizeof(float);  // tiles * NB == nmt * wcols
}

template <int CB, int MS, int NM, int EPI, bool BIAS, int MAXT, int KL>
int launch_gemm_kl(const GemmCfg &c, dim3 grid, size_t lds, hipStream_t s, const uint16_t *X, const uint16_t *W,
                   int m, int n, int k, const uint16_t *NWt, float eps, const float *ss_in, const uint16_t *Bs,
                   uint16_t *R, float *ss_out, uint16_t *Y, int ld, float *slab, int *ctr) {
    if (!lds_opt_in<&decode_gemm_kernel<CB, MS, NM, EPI, BIAS, MAXT, KL>>()) return SWH_E_LAUNCH;  // > 64 KB LDS
    decode_gemm_kernel<CB, MS, NM, EPI, BIAS, MAXT, KL><<<grid, 64u * c.nw, lds, s>>>(
        X, W, m, n, k, NWt, eps, ss_in, Bs, R, ss_out, Y, ld, slab, ctr, c.persist ? 1 : 0, c.wn, c.fw);
    return launch_status();
}

template <int CB, int MS, int NM, int EPI, bool BIAS, int MAXT>
int launch_gemm(const GemmCfg &c, dim3 grid, size_t lds, hipStream_t s, const uint16_t *X, const uint16_t *W, int m,
                int n, int k, const uint16_t *NWt, float eps, const float *ss_in, const uint16_t *Bs, uint16_t *R,
                float *ss_out, uint16_t *Y, int ld, float *slab, int *ctr) {
    // residual projections: o_proj (K = H) and down_proj (K = I) get distinct names
    if (EPI == EPI_RESIDUAL && k > 1024)
        return launch_gemm_kl<CB, MS, NM, EPI, BIAS, MAXT, 1>(c, grid, lds, s, X, W, m, n, k, NWt, eps, ss_in, Bs, R,
                                                              ss_out, Y, ld, slab, ctr);
    return launch_gemm_kl<CB, MS, NM, EPI, BIAS, MAXT, 0>(c, grid, lds, s, X, W, m, n, k, NWt, eps, ss_in, Bs, R,
                                                          ss_out, Y, ld, slab, ctr);
}

// the register-streamed short-K projection; 1 = not eligible
template <int KW, int MS, int NM, int EPI, bool BIAS>
int launch_xstream_kw(const GemmCfg &c, hipStream_t s, const uint16_t *X, const uint16_t *W, int m, int n, int k,
                      float eps, const float *ss_in, const uint16_t *Bs, uint16_t *R, float *ss_out, uint16_t *Y,
                      int ld) {
    xstream_gemm_kernel<KW, MS, NM, EPI, BIAS, 0><<<dim3((unsigned)c.gx), 512, 0, s>>>(X, W, m, n, k, eps, ss_in, Bs,
                                                                                    R, ss_out, Y, ld, c.fw, c.xf);
    return launch_status();
}

template <int MS, int NM, int EPI, bool BIAS>
int launch_xstream_ms(const GemmCfg &c, hipStream_t s, const uint16_t *X, const uint16_t *W, int m, int n, int k,
                      float eps, const float *ss_in, const uint16_t *Bs, uint16_t *R, float *ss_out, uint16_t *Y,
                      int ld) {
    const int ks = k / 32, kwn = (ks + 7) / 8;
    if (kwn <= 2) return launch_xstream_kw<2, MS, NM, EPI, BIAS>(c, s, X, W, m, n, k, eps, ss_in, Bs, R, ss_out, Y, ld);
    if (kwn <= 4) return launch_xstream_kw<4, MS, NM, EPI, BIAS>(c, s, X, W, m, n, k, eps, ss_in, Bs, R, ss_out, Y, ld);
    return launch_xstream_kw<8, MS, NM, EPI, BIAS>(c, s, X, W, m, n, k, eps, ss_in, Bs, R, ss_out, Y, ld);
}

int launch_xstream(const GemmCfg &c, hipStream_t s, const uint16_t *X, const uint16_t *W, int m, int n, int k, int nm,
                   float eps, const float *ss_in, const uint16_t *Bs, uint16_t *R, float *ss_out, uint16_t *Y, int ld) {
    const bool lds_image = !launch_policy().xstream;  // policy 0: decode_gemm_kernel's LDS image (A/B)
    const int ks = k / 32;
    if ((lds_image && !c.xf) || c.cb != 1 || c.wn != 1 || c.s != 1 || c.persist || c.nw != 8 || n % 16 ||
        ks < 8 || ks > (c.xf ? 152 : 64) || (c.ms != 1 && c.ms != 2))
        return 1;
    if (R) {  // o_proj: s += x W^T (+ the next norm's partial sums); down_proj over a fragment-order X
        if (nm != 0 || Bs || c.ms != 1) return 1;
        if (c.xf) {
            if (m % 16 || (ks + 7) / 8 > 19) return 1;
            if ((ks + 7) / 8 > 8)
                return launch_xstream_kw<19, 1, 0, EPI_RESIDUAL, false>(c, s, X, W, m, n, k, eps, nullptr, nullptr, R,
                                                                       ss_out, nullptr, ld);
        }
        return launch_xstream_ms<1, 0, EPI_RESIDUAL, false>(c, s, X, W, m, n, k, eps, nullptr, nullptr, R, ss_out, nullptr,
                                                            ld);
    }
    if (c.xf) return 1;
    if (nm != 2 || !ss_in || !Bs || !Y) return 1;  // qkv: folded norm + bias
    if (c.ms == 1)
        return launch_xstream_ms<1, 2, EPI_PLAIN, true>(c, s, X, W, m, n, k, eps, ss_in, Bs, nullptr, nullptr, Y, ld);
    return launch_xstream_ms<2, 2, EPI_PLAIN, true>(c, s, X, W, m, n, k, eps, ss_in, Bs, nullptr, nullptr, Y, ld);
}

template <int MS, int NM, int EPI, bool BIAS>
int launch_gemm_cb(const GemmCfg &c, dim3 grid, size_t lds, hipStream_t s, const uint16_t *X, const uint16_t *W,
                   int m, int n, int k, const uint16_t *NWt, float eps, const float *ss_in, const uint16_t *Bs,
                   uint16_t *R, float *ss_out, uint16_t *Y, int ld, float *slab, int *ctr) {
    switch (c.cb / c.wn) {  // column blocks per wave
    case 1:
        if (c.nw > 8)  // 16 waves: one-column-block tiles over long K
            return launch_gemm<1, MS, NM, EPI, BIAS, 1024>(c, grid, lds, s, X, W, m, n, k, NWt, eps, ss_in, Bs, R, ss_out, Y, ld, slab, ctr);
        return launch_gemm<1, MS, NM, EPI, BIAS, 512>(c, grid, lds, s, X, W, m, n, k, NWt, eps, ss_in, Bs, R, ss_out, Y, ld, slab, ctr);
    case 2: return launch_gemm<2, MS, NM, EPI, BIAS, 512>(c, grid, lds, s, X, W, m, n, k, NWt, eps, ss_in, Bs, R, ss_out, Y, ld, slab, ctr);
    default: return launch_gemm<4, MS, NM, EPI, BIAS, 512>(c, grid, lds, s, X, W, m, n, k, NWt, eps, ss_in, Bs, R, ss_out, Y, ld, slab, ctr);
    }
}

template <int NM, int EPI, bool BIAS>
int launch_gemm_ms(const GemmCfg &c, dim3 grid, size_t lds, hipStream_t s, const uint16_t *X, const uint16_t *W,
                   int m, int n, int k, const uint16_t *NWt, float eps, const float *ss_in, const uint16_t *Bs,
                   uint16_t *R, float *ss_out, uint16_t *Y, int ld, float *slab, int *ctr) {
    switch (c.ms) {
    case 1: return launch_gemm_cb<1, NM, EPI, BIAS>(c, grid, lds, s, X, W, m, n, k, NWt, eps, ss_in, Bs, R, ss_out, Y, ld, slab, ctr);
    case 2: return launch_gemm_cb<2, NM, EPI, BIAS>(c, grid, lds, s, X, W, m, n, k, NWt, eps, ss_in, Bs, R, ss_out, Y, ld, slab, ctr);
    default: return launch_gemm_cb<4, NM, EPI, BIAS>(c, grid, lds, s, X, W, m, n, k, NWt, eps, ss_in, Bs, R, ss_out, Y, ld, slab, ctr);
    }
}

}  // namespace
}  // namespace swh

using namespace swh;

extern "C" int64_t swh_decode_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K) {
    if (M <= 0 || N <= 0 || K <= 0) return kCounterBytes;
    int64_t a = wide_gemm_slab_bytes(M, N, K, 0), b = wide_gemm_slab_bytes(M, N, K, 1);
    for (int nrm : {0, 1, 2}) {
        const int64_t a1 = slab_bytes(pick_cfg(M, N, K, false, nrm), M, N);
        const int64_t b1 = slab_bytes(pick_cfg(M, 2 * N, K, true, nrm), M, 2 * N);
        a = a1 > a ? a1 : a;
        b = b1 > b ? b1 : b;
    }
    return kCounterBytes + (a > b ? a : b);
}

// fw: W in the swh_frag_pack layout (no norm_w, K % 128 == 0): the wide path
// reads row-major or its own packed weights only, so fw skips it
static int decode_gemm_impl(const void *x, const void *w, int64_t M, int64_t N, int64_t K, const void *norm_w,
                            float eps, const void *bias, void *residual, int32_t silu, void *y, int64_t ldy,
                            const float *ss_in, float *ss_out, void *workspace, int64_t workspace_bytes, void *stream,
                            int fw, int act = 0) {
    if (fw && (norm_w || K % 128)) return SWH_E_ARG;
    // act bit 0: the SiLU output in fragment order (tile path only); bit 1: X in fragment order (xstream only)
    if (act & ~3 || ((act & 1) && (!silu || N % 32 || M % 16)) || ((act & 2) && (!residual || M % 16 || K % 32)))
        return SWH_E_ARG;
    if (!x || !w || M <= 0 || N <= 0 || K <= 0 || K % 64 || M > (1 << 20) || N >= (1 << 29) || K >= (1 << 29))
        return SWH_E_ARG;
    if (residual && (silu || bias)) return SWH_E_ARG;
    if (!residual && !y) return SWH_E_ARG;
    if (ss_in && !norm_w && residual) return SWH_E_ARG;  // folded-norm row scale: plain / SiLU epilogues
    if (ss_out && !residual) return SWH_E_ARG;
    if (N % (silu ? 8 : 16) || ldy % 8 || ldy < N) return SWH_E_ARG;
    const uintptr_t out_ptr = reinterpret_cast<uintptr_t>(residual ? residual : y);
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w) | out_ptr) & 15) return SWH_E_ARG;
    if ((bias && (reinterpret_cast<uintptr_t>(bias) & 15)) || (norm_w && (reinterpret_cast<uintptr_t>(norm_w) & 15)) ||
        (ss_in && (reinterpret_cast<uintptr_t>(ss_in) & 15)))
        return SWH_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t wcols = silu ? 2 * N : N;
    const int nm = norm_w ? 1 : (ss_in ? 2 : 0);
    const swh_launch_policy pol = launch_policy();
    if (!fw && nm != 1 && K >= pol.wide_kmin && pol.wide_gemm) {  // the bandwidth regime (8B decode): csrc/wide_gemm.hip
        const int st = wide_gemm(x, w, M, N, K, eps, ss_in, bias, residual, silu, y, ldy, ss_out, workspace,
                                 workspace_bytes, kCounterBytes, 0, s);
        if (st != 1) return st;
    }
    {  // many 16-column tiles and a K that fits the X image: the tile kernel (lm head, gate/up)
        const int64_t ntile = silu ? N / 8 : N / 16;
        const bool force = pol.gemm_tile != 0, overridden = pol.gemm_ms != 0;  // policy: force / bypass the tile kernel
        // gate/up (SiLU tiles) from one tile per CU up: 11.2 vs 12.4 us at N 9728 (tools/bench_decode.py --ku)
        const int64_t min_tiles = (silu ? 1 : 8) * (int64_t)cu_count();
        // (the epilogues store 8 columns of a row as one 16-B piece: row-major needs ldy % 8 == 0)
        if (!residual && K <= 32 * kLmMaxKS && (force || (!overridden && ntile >= min_tiles)) &&
            ((silu && (act & 1)) || ldy % 8 == 0)) {
            const int64_t nmt = (M + 63) / 64;
            const GemmLds L = gemm_lds(1, 64, 8, (int)K, (int)K, nm, false);
            int64_t per = cu_count() / nmt > 0 ? cu_count() / nmt : 1;
            if (per > ntile) per = ntile;
            const dim3 grid((unsigned)(per * nmt));
            const auto *X = static_cast<const uint16_t *>(x);
            const auto *W = static_cast<const uint16_t *>(w);
            const auto *NWt = static_cast<const uint16_t *>(norm_w);
            const auto *Bs = static_cast<const uint16_t *>(bias);
            auto *Y = static_cast<uint16_t *>(y);
            const size_t lds = (size_t)L.total + (silu ? 8 : 16) * 1024;  // + the epilogue's 1 / 2 KB per wave
            if (silu) return tile_gemm(EPI_SILU, nm, grid, lds, s, X, W, (int)M, (int)N, (int)K, NWt, eps, ss_in, Bs, Y, (int)ldy, fw, act & 1);
            return tile_gemm(EPI_PLAIN, nm, grid, lds, s, X, W, (int)M, (int)N, (int)K, NWt, eps, ss_in, Bs, Y, (int)ldy, fw, 0);
        }
    }
    if (act & 1) return SWH_E_ARG;  // the fragment-order SiLU output comes from the tile kernel only
    GemmCfg c = pick_cfg(M, wcols, K, silu != 0, nm);
    c.fw = fw;
    c.xf = (act & 2) ? 1 : 0;
    const int64_t MR = 16 * c.ms, nmt = (M + MR - 1) / MR, ncb = wcols / (16 * c.cb);
    // workspace: [counters (zeroed once, self-resetting) | fp32 slabs]
    int *ctr = static_cast<int *>(workspace);
    float *slab = nullptr;
    if (c.s > 1) {
        if (ncb * nmt * (int64_t)sizeof(int) > kCounterBytes) return SWH_E_ARG;
        if (!workspace || workspace_bytes < kCounterBytes + slab_bytes(c, M, wcols)) return SWH_E_ARG;
        // counters live in a FIXED region at the start (never overlapped by any
        // call's slabs, whatever its shape), so a self-reset counter stays zero
        slab = reinterpret_cast<float *>(static_cast<char *>(workspace) + kCounterBytes);
    }
    const auto *X = static_cast<const uint16_t *>(x);
    const auto *W = static_cast<const uint16_t *>(w);
    const auto *NWt = static_cast<const uint16_t *>(norm_w);
    const auto *Bs = static_cast<const uint16_t *>(bias);
    auto *R = static_cast<uint16_t *>(residual);
    auto *Y = static_cast<uint16_t *>(y);
    const int m = (int)M, n = (int)N, k = (int)K, ld = (int)ldy;
    const GemmLds L = gemm_lds(c.cb, (int)MR, c.nw, (int)((K / 32 + c.s - 1) / c.s * 32), (int)K, nm, c.persist,
                               c.wn);
    if (L.total > 160 * 1024 || c.gx <= 0) return SWH_E_ARG;
    const dim3 grid((unsigned)c.gx, 1u, (unsigned)c.s);
    const size_t lds = (size_t)L.total;
#define SWH_GEMM(NORM_, EPI_, BIAS_) \
    return launch_gemm_ms<NORM_, EPI_, BIAS_>(c, grid, lds, s, X, W, m, n, k, NWt, eps, ss_in, Bs, R, ss_out, Y, ld, slab, ctr)
    if (silu) {
        if (nm == 1) SWH_GEMM(1, EPI_SILU, false);
        if (nm == 2) SWH_GEMM(2, EPI_SILU, false);
        SWH_GEMM(0, EPI_SILU, false);
    }
    if (residual) {
        if (nm == 0) {
            const int rc = launch_xstream(c, s, X, W, m, n, k, nm, eps, ss_in, Bs, R, ss_out, nullptr, ld);
            if (rc != 1) return rc;
        }
        if (c.xf) return SWH_E_ARG;  // a fragment-order X is read by xstream only
        if (nm == 1) SWH_GEMM(1, EPI_RESIDUAL, false);
        SWH_GEMM(0, EPI_RESIDUAL, false);
    }
    if (Bs) {
        if (nm == 1) SWH_GEMM(1, EPI_PLAIN, true);
        if (nm == 2) {
            const int rc = launch_xstream(c, s, X, W, m, n, k, nm, eps, ss_in, Bs, nullptr, nullptr, Y, ld);
            if (rc != 1) return rc;
            SWH_GEMM(2, EPI_PLAIN, true);
        }
        SWH_GEMM(0, EPI_PLAIN, true);
    }
    if (nm == 1) SWH_GEMM(1, EPI_PLAIN, false);
    if (nm == 2) SWH_GEMM(2, EPI_PLAIN, false);
    SWH_GEMM(0, EPI_PLAIN, false);
#undef SWH_GEMM
}

extern "C" int swh_decode_gemm(const void *x, const void *w, int64_t M, int64_t N, int64_t K, const void *norm_w,
                               float eps, const void *bias, void *residual, int32_t silu, void *y, int64_t ldy,
                               const float *ss_in, float *ss_out, void *workspace, int64_t workspace_bytes,
                               void *stream) {
    return decode_gemm_impl(x, w, M, N, K, norm_w, eps, bias, residual, silu, y, ldy, ss_in, ss_out, workspace,
                            workspace_bytes, stream, 0);
}

extern "C" int swh_decode_gemm_fragw(const void *x, const void *w, int64_t M, int64_t N, int64_t K, float eps,
                                     const void *bias, void *residual, int32_t silu, void *y, int64_t ldy,
                                     const float *ss_in, float *ss_out, int32_t act_frag, void *workspace,
                                     int64_t workspace_bytes, void *stream) {
    return decode_gemm_impl(x, w, M, N, K, nullptr, eps, bias, residual, silu, y, ldy, ss_in, ss_out, workspace,
                            workspace_bytes, stream, 1, act_frag);
}

extern "C" int swh_frag_pack(const void *w, const void *norm_w, int64_t N, int64_t K, int32_t silu, void *dst,
                             void *stream) {
    const int64_t rows = silu ? 2 * N : N;
    if (!w || !dst || w == dst || N <= 0 || rows % 16 || (silu && N % 8) || K <= 0 || K % 128) return SWH_E_ARG;
    if ((reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(norm_w)) & 15)
        return SWH_E_ARG;
    return frag_pack(w, norm_w, N, K, silu, dst, static_cast<hipStream_t>(stream));
}
