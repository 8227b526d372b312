// Attention of the decode step (GQA), flash-decoding form — one workgroup (8 waves) per
// (kv head, sequence): every lane issues the K and V loads of up to J keys
// before the RoPE prologue, so the KV stream is one round trip; scores,
// online softmax and P.V stay in registers, lanes/waves merge (m, l, acc).
//
// Here: attn_decode_kernel, the row-pair form for D = 128 (attn_decode_pair_kernel), the
// Infinity Cache warm-up their spare grid rows run, and the swh_attn_decode* entry points.
#include "decode_common.hpp"

namespace swh {
namespace {

// Infinity Cache warm-up job: a device range read (and discarded) by warm-up workgroups
struct L3Job {
    const uint4 *p;
    int64_t n16;       // 16-B units
    int64_t reserved;  // 0
};
constexpr int kL3MaxJobs = 8;

// warm-up workgroup p of npf (NT threads): a contiguous share of the jobs' bytes,
// 8 x 16-B loads in flight per thread, XOR-ed into a word stored only if it
// equals a magic constant
template <int NT>
__device__ __forceinline__ void l3_warm_share(const L3Job *__restrict__ jobs, int njobs, int p, int npf,
                                              uint32_t *__restrict__ sink) {
    const int tid = threadIdx.x;
    int64_t tot = 0;
    for (int j = 0; j < njobs; ++j) tot += jobs[j].n16;
    const int64_t share = (tot + npf - 1) / npf, lo = (int64_t)p * share, hi = min(tot, lo + share);
    uint32_t acc = 0;
    auto sweep = [&](const uint4 *src, int64_t a, int64_t e) {
        for (int64_t i = a + tid; i < e; i += 8 * NT) {
            uint4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int64_t q = i + u * NT;
                v[u] = q < e ? src[q] : uint4{0u, 0u, 0u, 0u};
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) acc ^= v[u].x ^ v[u].y ^ v[u].z ^ v[u].w;
        }
    };
    int64_t base = 0;
    for (int j = 0; j < njobs; ++j) {
        const int64_t n = jobs[j].n16;
        sweep(jobs[j].p, max(lo - base, (int64_t)0), min(hi - base, n));
        base += n;
    }
    if (acc == 0x9e3779b9u) sink[(int64_t)p * NT + tid] = acc;
}

// ---------------------------------------------------------------------------
// Attention decode (GQA) on MFMA, swapped orientation: one workgroup (8 waves)
// per (kv head, sequence).  S^T = K Q^T on v_mfma_f32_16x16x32_bf16 (A = 16
// cached keys straight from HBM, B = the GQ <= 16 query heads, zero-padded),
// so each lane holds ONE head (lane & 15) and four keys: the softmax max / sum
// reduce over registers and two lane groups only, and P^T, packed to bf16
// pairwise, is the B operand of O^T = V^T P^T as it stands (no LDS round
// trip).  V^T comes from the wave's V tile in LDS through ds_read_b64_tr_b16
// (4 keys x 1 dim per lane).  Waves take interleaved 16-key blocks; every K/V
// load of a round is issued before the RoPE prologue.
// ---------------------------------------------------------------------------
typedef short bf16x4s __attribute__((ext_vector_type(4)));
// Threads of a decode-attention workgroup (one (kv head, row)).  At D = 128 (Llama-3-8B:
// 512 workgroups, 164 VGPRs) four waves let two workgroups share a CU, so one streams
// while the other runs its prologue / merge: 41.3 -> 37.4 us per layer, decode step
// 4857 -> 4737 us (two waves: 42.7, three: 38.1; profiles/r5_att4w_graph.log,
// r5_att2w_graph.log).  At D = 64 (the 0.5B bench, 128 workgroups) eight.
constexpr int attn_threads(int D) { return D == 128 ? 256 : 512; }

__device__ __forceinline__ bf16x4s lds_read_tr16(const uint16_t *p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) bf16x4s *)(const_cast<uint16_t *>(p)));
}

// Per-launch options of the decode attention.  The attention grid covers only
// Hkv x B workgroups (128 of 256 CUs at the bench shape); with `jobs`, extra grid
// rows read the weights of the projections that follow into the Infinity Cache
// (swh_attn_decode_l3) and exit.
struct AttnPrefetch {
    int rows;              // attention rows (B): grid rows past it warm the cache
    const int32_t *prow;   // [B] row whose cache holds this row's prompt keys / values, or null (own row)
    int ofrag = 0;         // output in the fragment order o_proj's register-streamed A operand reads (B % 16 == 0)
    const L3Job *jobs = nullptr;  // Infinity Cache warm-up ranges (grid rows past `rows` read them), or null
    int njobs = 0;
    uint32_t *sink = nullptr;     // >= warm-up workgroups x 512 words, written never in practice
    int nwg = 0;                  // warm-up workgroups wanted (rounded up to whole grid rows)
};

// element (row b, column c) of a [B, K] activation in the fragment order of
// xstream_gemm_kernel's A operand (the act_frag layout): per 16-row group and
// 32-wide k-step one 1 KB run of 64 lanes x 8 consecutive columns
__device__ __forceinline__ int64_t frag_at(int64_t b, int c, int K) {
    return (((b >> 4) * (K >> 5) + (c >> 5)) * 64 + ((c >> 3) & 3) * 16 + (b & 15)) * 8 + (c & 7);
}

// Occupancy at D = 128 (Llama-3-8B), measured (profiles/r5_att_ab.log): 164 VGPRs.  With
// eight waves one workgroup per CU; two per CU by a 128-VGPR bound spill (62 us against
// 41.5 us per launch, Q fragments re-read from LDS 60 us); 4 key blocks per wave per
// round (256 VGPRs) 44.8 us.  Four-wave workgroups (attn_threads) put two on a CU
// without either: 37.4 us.
template <int D, int GQ>
__global__ __launch_bounds__(attn_threads(D)) void attn_decode_kernel(
    const uint16_t *__restrict__ qkv, uint16_t *__restrict__ kc, uint16_t *__restrict__ vc,
    const float *__restrict__ rcos, const float *__restrict__ rsin, const int32_t *__restrict__ plen,
    const int32_t *__restrict__ state, int Hq, int Hkv, int Tmax, float scale, uint16_t *__restrict__ out,
    AttnPrefetch pf) {
    static_assert(GQ <= 16, "a kv head serves at most 16 query heads");
    constexpr int kAttnThreads = attn_threads(D), kAttnWaves = kAttnThreads / 64;
    constexpr int DC = D / 32;                 // 32-dim chunks: k-steps of K Q^T
    constexpr int DB = D / 16;                 // 16-dim blocks of O^T
    constexpr int JB = (D == 64) ? 4 : 2;      // key blocks per wave per round (pairs for P V)
    constexpr int KPR = JB * 16 * kAttnWaves;  // keys per round
    constexpr int HD = D / 2;
    constexpr int VS = D + (D == 64 ? 8 : 16);  // V tile row stride (elements): conflict-free transposed reads
    __shared__ __attribute__((aligned(16))) uint16_t q_s[16 * D];
    __shared__ __attribute__((aligned(16))) uint16_t kn_s[D];
    __shared__ __attribute__((aligned(16))) uint16_t vn_s[D];
    // a wave's V tile (its key loop) and, after its loop, its (acc, m, l) record for the
    // merge share one LDS slot: 2 workgroups per CU fit at D = 128 (78 KB instead of 144)
    constexpr int kRed = 16 * (D + 2) * 4, kVt = 32 * VS * 2;
    constexpr int kSlot = (kRed > kVt ? kRed : kVt) / 16 * 16;
    __shared__ __attribute__((aligned(16))) unsigned char slot_s[kAttnWaves][kSlot];
    auto red_s = [&](int w2, int h) -> float * { return reinterpret_cast<float *>(slot_s[w2]) + h * (D + 2); };

    const int kvh = blockIdx.x;
    const int64_t b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int g = lane >> 4, c16 = lane & 15;
    SWH_GEMM_TRACE(0);  // phase stamps for tools/attn_probe.py (instrumented build only)
    if ((int)blockIdx.y >= pf.rows) {  // an Infinity Cache warm-up workgroup
        if (pf.jobs)
            l3_warm_share<kAttnThreads>(pf.jobs, pf.njobs, (blockIdx.y - pf.rows) * gridDim.x + blockIdx.x,
                                        (gridDim.y - pf.rows) * gridDim.x, pf.sink);
        return;
    }
    // state[0] = index of the token sampled this step; the input token is state[0] - 1
    const int step = state[0] - 1, P = state[1];
    const int pl = plen[b];
    const int slot_new = P + step;
    const int start = P - pl;
    const int pos = pl + step;
    uint16_t *ob = out + b * (int64_t)Hq * D + kvh * GQ * D;
    if (step < 0 || slot_new >= Tmax || pl < 0 || pl > P) {  // never write outside the cache
        for (int idx = tid; idx < GQ * D; idx += kAttnThreads)  // NaN: fail loudly
            out[pf.ofrag ? frag_at(b, kvh * GQ * D + idx, Hq * D) : b * (int64_t)Hq * D + kvh * GQ * D + idx] = 0x7fc0;
        return;
    }
    const int n = slot_new - start + 1;  // keys incl. the new one (index n-1)
    const int64_t cbase = (b * Hkv + kvh) * (int64_t)Tmax * D;
    const uint16_t *kb = kc + cbase + (int64_t)start * D + g * 8;
    const uint16_t *vb = vc + cbase + (int64_t)start * D + g * 8;
    // prompt keys (index < pl, slots start .. P-1) from the row that holds the group's prompt:
    // the G rows of a GRPO group read one copy (HBM once, the rest from the caches)
    const int64_t prow = pf.prow ? (int64_t)min(max(pf.prow[b], 0), pf.rows - 1) : b;
    const int64_t pbase = (prow * Hkv + kvh) * (int64_t)Tmax * D;
    const uint16_t *kbp = kc + pbase + (int64_t)start * D + g * 8;
    const uint16_t *vbp = vc + pbase + (int64_t)start * D + g * 8;

    // lane (g, c16) loads key c16 of each block, dims 32 c + 8 g: the A fragment of K Q^T
    u32x4 kr[JB][DC], vr[JB][DC];  // vector types: uint4 structs defeat SROA under selects
#define SWH_ATTN_ISSUE(base_)                                                                  \
    _Pragma("unroll") for (int i = 0; i < JB; ++i) {                                           \
        const int k0_ = (base_) + (wid + i * kAttnWaves) * 16;                                 \
        if (k0_ < n) {                                                                         \
            const int kk = max(min(k0_ + c16, n - 2), 0);                                      \
            const uint16_t *ks_ = kk < pl ? kbp : kb, *vs_ = kk < pl ? vbp : vb;               \
            _Pragma("unroll") for (int c = 0; c < DC; ++c) {                                   \
                kr[i][c] = *reinterpret_cast<const u32x4 *>(ks_ + (int64_t)kk * D + c * 32);   \
                vr[i][c] = *reinterpret_cast<const u32x4 *>(vs_ + (int64_t)kk * D + c * 32);   \
            }                                                                                  \
        }                                                                                      \
    }
    SWH_ATTN_ISSUE(0)  // the KV stream is in flight during RoPE
    SWH_GEMM_TRACE(1);

    const uint16_t *row = qkv + b * (int64_t)(Hq + 2 * Hkv) * D;
    for (int idx = tid; idx < (GQ + 1) * HD; idx += kAttnThreads) {
        const int hh = idx / HD, i = idx - hh * HD;
        const float c = rcos[(int64_t)pos * HD + i], s = rsin[(int64_t)pos * HD + i];
        const uint16_t *src = (hh < GQ) ? row + (kvh * GQ + hh) * D : row + (Hq + kvh) * D;
        const float x1 = bf16_bits_to_f32(src[i]), x2 = bf16_bits_to_f32(src[i + HD]);
        const uint16_t o1 = f32_to_bf16_bits(round_bf16(x1 * c) + round_bf16(-x2 * s));
        const uint16_t o2 = f32_to_bf16_bits(round_bf16(x2 * c) + round_bf16(x1 * s));
        if (hh < GQ) {
            q_s[hh * D + i] = o1;
            q_s[hh * D + i + HD] = o2;
        } else {
            kn_s[i] = o1;
            kn_s[i + HD] = o2;
        }
    }
    for (int idx = GQ * D + tid; idx < 16 * D; idx += kAttnThreads) q_s[idx] = 0;
    for (int d = tid; d < D; d += kAttnThreads) vn_s[d] = row[(Hq + Hkv + kvh) * D + d];
    lds_barrier();
    SWH_GEMM_TRACE(2);
    for (int d = tid; d < D; d += kAttnThreads) {  // KV append (nobody reads the slot from memory this step)
        kc[cbase + (int64_t)slot_new * D + d] = kn_s[d];
        vc[cbase + (int64_t)slot_new * D + d] = vn_s[d];
    }

    // B operand of K Q^T: lane holds head c16, dims 32 c + 8 g
    u32x4 qb[DC];
#pragma unroll
    for (int c = 0; c < DC; ++c) qb[c] = *reinterpret_cast<const u32x4 *>(q_s + c16 * D + c * 32 + g * 8);
    float m = kNegInf, l = 0.f;  // of head c16
    f32x4 o[DB];                 // O^T: dims 16 db + 4 g + r, head c16
#pragma unroll
    for (int d = 0; d < DB; ++d) o[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    uint16_t *vt = reinterpret_cast<uint16_t *>(slot_s[wid]);

    for (int base = 0; base < n; base += KPR) {
        if (base) {
            SWH_ATTN_ISSUE(base)
        }
        f32x4 sc[JB];  // S^T: keys k0 + 4 g + r, head c16
        float mx = m;
#pragma unroll
        for (int i = 0; i < JB; ++i) {
            const int k0 = base + (wid + i * kAttnWaves) * 16;
            sc[i] = f32x4{kNegInf, kNegInf, kNegInf, kNegInf};
            if (k0 < n) {  // wave-uniform
                const bool fresh = (k0 + c16 == n - 1);  // the new key/value: from LDS, not the cache
#pragma unroll
                for (int c = 0; c < DC; ++c) {
                    const u32x4 kn = *reinterpret_cast<const u32x4 *>(kn_s + c * 32 + g * 8);
                    const u32x4 vn = *reinterpret_cast<const u32x4 *>(vn_s + c * 32 + g * 8);
                    kr[i][c] = fresh ? kn : kr[i][c];
                    vr[i][c] = fresh ? vn : vr[i][c];
                }
                f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < DC; ++c)
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kr[i][c]),
                                                                  __builtin_bit_cast(bf16x8, qb[c]), acc, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    sc[i][r] = (k0 + 4 * g + r < n) ? acc[r] * scale : kNegInf;
                    mx = fmaxf(mx, sc[i][r]);
                }
            }
        }
        // online softmax of head c16: its keys sit in 4 registers x JB blocks x the 4 lane groups
        mx = fmaxf(mx, __shfl_xor(mx, 16, kWave));
        mx = fmaxf(mx, __shfl_xor(mx, 32, kWave));
        const float corr = (mx == kNegInf) ? 1.f : expf(m - mx);
        l *= corr;
#pragma unroll
        for (int d = 0; d < DB; ++d) o[d] *= corr;
        m = mx;
        // P V: blocks in pairs -> 32 keys per MFMA; P^T (bf16 pairs) is the B operand as it stands
#pragma unroll
        for (int i = 0; i < JB; i += 2) {
            const int k0 = base + (wid + i * kAttnWaves) * 16;
            const int k1 = base + (wid + (i + 1) * kAttnWaves) * 16;
            if (k0 < n) {  // wave-uniform
                float pj[8];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    pj[r] = (mx == kNegInf) ? 0.f : expf(sc[i][r] - mx);
                    pj[4 + r] = (mx == kNegInf) ? 0.f : expf(sc[i + 1][r] - mx);
                    l += pj[r] + pj[4 + r];
                }
                // the pair's V rows into the wave's tile (rows 0-15: block i, 16-31: block i+1; zeros past n)
#pragma unroll
                for (int c = 0; c < DC; ++c) {
                    *reinterpret_cast<u32x4 *>(vt + c16 * VS + c * 32 + g * 8) = vr[i][c];
                    *reinterpret_cast<u32x4 *>(vt + (16 + c16) * VS + c * 32 + g * 8) =
                        (k1 < n) ? vr[i + 1][c] : u32x4{0u, 0u, 0u, 0u};
                }
                uint32_t pb[4];
#pragma unroll
                for (int h = 0; h < 4; ++h)
                    pb[h] = __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{pj[2 * h], pj[2 * h + 1]}, bf16x2));
                const bf16x8 pbf = __builtin_bit_cast(bf16x8, u32x4{pb[0], pb[1], pb[2], pb[3]});
                // V^T fragment: lane (g, c16) <- dims 16 db + c16 of keys {4 g .. 4 g + 3} and {16 + 4 g ..}
                const int q = c16 >> 2, pq = c16 & 3;
#pragma unroll
                for (int d = 0; d < DB; ++d) {
                    const bf16x4s lo = lds_read_tr16(vt + (4 * g + q) * VS + d * 16 + 4 * pq);
                    const bf16x4s hi = lds_read_tr16(vt + (16 + 4 * g + q) * VS + d * 16 + 4 * pq);
                    const bf16x8 va = __builtin_bit_cast(
                        bf16x8, u32x4{__builtin_bit_cast(uint2, lo).x, __builtin_bit_cast(uint2, lo).y,
                                      __builtin_bit_cast(uint2, hi).x, __builtin_bit_cast(uint2, hi).y});
                    o[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pbf, o[d], 0, 0, 0);
                }
            }
        }
    }
    SWH_GEMM_TRACE(3);
    // row sums across the 4 lane groups, then the waves merge through LDS (the record
    // overwrites this wave's own V tile: its last transposed reads must retire first)
    l += __shfl_xor(l, 16, kWave);
    l += __shfl_xor(l, 32, kWave);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    float *rec = red_s(wid, c16);
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int r = 0; r < 4; ++r) rec[d * 16 + 4 * g + r] = o[d][r];
    if (g == 0) {
        rec[D] = m;
        rec[D + 1] = l;
    }
    __syncthreads();
    SWH_GEMM_TRACE(4);
    auto merged = [&](int h, int d) -> uint16_t {  // the waves' (m, l, acc) of head h, dim d
        float mxw = kNegInf;
#pragma unroll
        for (int w2 = 0; w2 < kAttnWaves; ++w2) mxw = fmaxf(mxw, red_s(w2, h)[D]);
        float Ls = 0.f, A = 0.f;
#pragma unroll
        for (int w2 = 0; w2 < kAttnWaves; ++w2) {
            const float *rw = red_s(w2, h);
            const float mq = rw[D];
            if (mq == kNegInf) continue;
            const float cq = expf(mq - mxw);
            Ls = fmaf(rw[D + 1], cq, Ls);
            A = fmaf(rw[d], cq, A);
        }
        return f32_to_bf16_bits(A / Ls);
    };
    if (pf.ofrag) {
        // one element per thread as below; lanes 8j .. 8j+7 hold 8 consecutive dims
        // (GQ * D % 64 == 0: whole waves per pass), gathered by shuffles into lane 8j,
        // which stores them as one 16-B piece at their fragment-order place
        for (int idx = tid; idx < GQ * D; idx += kAttnThreads) {
            const int h = idx / D, d = idx - h * D;
            const uint32_t v = merged(h, d);
            const uint32_t p2 = v | (__shfl_down(v, 1, kWave) << 16);
            const uint32_t p4 = __shfl_down(p2, 2, kWave);
            const uint32_t p6 = __shfl_down(p2, 4, kWave), p8 = __shfl_down(p2, 6, kWave);
            if ((lane & 7) == 0)
                *reinterpret_cast<uint4 *>(out + frag_at(b, (kvh * GQ + h) * D + d, Hq * D)) = uint4{p2, p4, p6, p8};
        }
    } else {
        for (int idx = tid; idx < GQ * D; idx += kAttnThreads) {
            const int h = idx / D, d = idx - h * D;
            ob[idx] = merged(h, d);
        }
    }
    SWH_GEMM_TRACE(5);
#undef SWH_ATTN_ISSUE
}

// ---------------------------------------------------------------------------
// Row-pair decode attention (D = 128, 2 GQ <= 16: Llama-3-8B): one 8-wave workgroup
// per (kv head, two consecutive rows).  The MFMA's 16 query columns hold both rows'
// heads (row A in columns 0 .. GQ-1, row B in GQ .. 2 GQ-1), so when the rows share a
// GRPO group's prompt (prompt_row and prompt length equal) its keys and values are
// loaded ONCE and scored for both rows; each row's own keys follow with the other
// row's columns masked to -inf (their online-softmax state untouched).  One wave of
// 256 workgroups instead of two of 512 halves the exposed argument / RoPE / merge
// phases as well (timing probe: 37.8 -> 32.3 us per layer, profiles/r5_pair_graph.log).
// Same per-column arithmetic as attn_decode_kernel (scores, online softmax, P V,
// fixed-order wave merge), with the keys visited in another order.
// ---------------------------------------------------------------------------
template <int D, int GQ>
__global__ __launch_bounds__(512) void attn_decode_pair_kernel(
    const uint16_t *__restrict__ qkv, uint16_t *__restrict__ kc, uint16_t *__restrict__ vc,
    const float *__restrict__ rcos, const float *__restrict__ rsin, const int32_t *__restrict__ plen,
    const int32_t *__restrict__ state, int Hq, int Hkv, int Tmax, float scale, uint16_t *__restrict__ out,
    AttnPrefetch pf) {
    static_assert(2 * GQ <= 16, "two rows' query heads in the 16 MFMA columns");
    constexpr int NT = 512, NW = NT / 64;
    constexpr int DC = D / 32, DB = D / 16, JB = 2, KPR = JB * 16 * NW, HD = D / 2;
    constexpr int VS = D + (D == 64 ? 8 : 16);
    __shared__ __attribute__((aligned(16))) uint16_t q_s[16 * D];
    __shared__ __attribute__((aligned(16))) uint16_t kn_s[2][D];
    __shared__ __attribute__((aligned(16))) uint16_t vn_s[2][D];
    constexpr int kRed = 16 * (D + 2) * 4, kVt = 32 * VS * 2;
    constexpr int kSlot = (kRed > kVt ? kRed : kVt) / 16 * 16;
    __shared__ __attribute__((aligned(16))) unsigned char slot_s[NW][kSlot];
    auto red_s = [&](int w2, int h) -> float * { return reinterpret_cast<float *>(slot_s[w2]) + h * (D + 2); };

    const int kvh = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int g = lane >> 4, c16 = lane & 15;
    const int npairs = (pf.rows + 1) / 2;
    if ((int)blockIdx.y >= npairs) {  // an Infinity Cache warm-up workgroup
        if (pf.jobs)
            l3_warm_share<NT>(pf.jobs, pf.njobs, (blockIdx.y - npairs) * gridDim.x + blockIdx.x,
                              (gridDim.y - npairs) * gridDim.x, pf.sink);
        return;
    }
    const int step = state[0] - 1, P = state[1];
    const int slot_new = P + step;
    // never write outside the cache: a row with an out-of-range length or step gets NaN
    // (fails loudly) and no KV append; its partner row still runs, alone
    const int64_t b0 = 2 * (int64_t)blockIdx.y;
    const bool has1 = b0 + 1 < pf.rows;
    const int pl0 = plen[b0], pl1 = has1 ? plen[b0 + 1] : 0;
    const bool ok0 = !(step < 0 || slot_new >= Tmax || pl0 < 0 || pl0 > P);
    const bool ok1 = has1 && !(step < 0 || slot_new >= Tmax || pl1 < 0 || pl1 > P);
    for (int r = 0; r < (has1 ? 2 : 1); ++r) {
        if (r ? ok1 : ok0) continue;
        const int64_t b = b0 + r;
        for (int idx = tid; idx < GQ * D; idx += NT)
            out[pf.ofrag ? frag_at(b, kvh * GQ * D + idx, Hq * D) : b * (int64_t)Hq * D + kvh * GQ * D + idx] = 0x7fc0;
    }
    if (!ok0 && !ok1) return;
    const int64_t bA = ok0 ? b0 : b0 + 1;
    const bool hasB = ok0 && ok1;
    const int64_t bB = hasB ? bA + 1 : bA;
    const int plA = ok0 ? pl0 : pl1, plB = hasB ? pl1 : plA;
    const int64_t prA = pf.prow ? (int64_t)min(max(pf.prow[bA], 0), pf.rows - 1) : bA;
    const int64_t prB = pf.prow ? (int64_t)min(max(pf.prow[bB], 0), pf.rows - 1) : bB;
    const bool shared = hasB && prA == prB && plA == plB && plA > 0;  // one prompt for both rows
    const int nA = slot_new - (P - plA) + 1, nB = slot_new - (P - plB) + 1;  // keys incl. the new one
    auto cbase = [&](int64_t r) -> int64_t { return (r * Hkv + kvh) * (int64_t)Tmax * D; };
    const int64_t cbA = cbase(bA), cbB = cbase(bB);

    // key segments: [lo, hi) of a row's key numbering (prompt keys first), read from the
    // prompt row's cache below pl and the row's own cache from pl on; columns [clo, chi)
    struct Seg {
        int lo, hi, pl, n, clo, chi, fresh;  // fresh: 0 none, 1 row A's new key, 2 row B's
        const uint16_t *kb, *vb, *kbp, *vbp;
    };
    const int stA = P - plA, stB = P - plB;
    const uint16_t *kA = kc + cbA + (int64_t)stA * D + g * 8, *vA = vc + cbA + (int64_t)stA * D + g * 8;
    const uint16_t *kB = kc + cbB + (int64_t)stB * D + g * 8, *vB = vc + cbB + (int64_t)stB * D + g * 8;
    const uint16_t *kpA = kc + cbase(prA) + (int64_t)stA * D + g * 8, *vpA = vc + cbase(prA) + (int64_t)stA * D + g * 8;
    const uint16_t *kpB = kc + cbase(prB) + (int64_t)stB * D + g * 8, *vpB = vc + cbase(prB) + (int64_t)stB * D + g * 8;
    // A row's keys are always visited as its prompt [0, pl), then its own [pl, n), with the
    // same round boundaries, so a column's result does not depend on whether the pair
    // shares its prompt (shared: one prompt segment scored for both rows' columns).  No
    // dynamic indexing (a segment array lived in scratch): the segments as values.
    const Seg sP{0, plA, plA, 0x7fffffff, 0, 2 * GQ, 0, kA, vA, kpA, vpA};
    const Seg sAp{0, plA, plA, 0x7fffffff, 0, GQ, 0, kA, vA, kpA, vpA};
    const Seg sAo{plA, nA, plA, nA, 0, GQ, 1, kA, vA, kpA, vpA};
    const Seg sBp{0, hasB ? plB : 0, plB, 0x7fffffff, GQ, 2 * GQ, 0, kB, vB, kpB, vpB};
    const Seg sBo{plB, hasB ? nB : plB, plB, nB, GQ, 2 * GQ, 2, kB, vB, kpB, vpB};
    const Seg s0 = shared ? sP : sAp;

    u32x4 kr[JB][DC], vr[JB][DC];
    // A run visits the 16-key blocks of a virtual list: part X's keys [X.lo, X.hi) padded to
    // whole blocks, then part Y's [Y.lo, Y.hi); each block belongs to one part (wave-uniform),
    // so both rows' own keys share rounds.  blk(k0v) -> the part's Seg and key index.
#define SWH_PAIR_BLOCK(X_, Y_, k0v_, S_, k0_)                                                     \
    const int p1_ = ((X_).hi - (X_).lo + 15) / 16 * 16;                                           \
    const bool iny_ = (k0v_) >= p1_;                                                              \
    const Seg S_ = iny_ ? (Y_) : (X_);                                                            \
    const int k0_ = iny_ ? (Y_).lo + (k0v_) - p1_ : (X_).lo + (k0v_);
#define SWH_PAIR_ISSUE(X_, Y_, base_)                                                             \
    _Pragma("unroll") for (int i = 0; i < JB; ++i) {                                              \
        SWH_PAIR_BLOCK(X_, Y_, (base_) + (wid + i * NW) * 16, S_, k0_)                            \
        if (k0_ < S_.hi) {                                                                        \
            const int kk = max(min(k0_ + c16, min(S_.hi, S_.n - 1) - 1), 0);                      \
            const uint16_t *ks_ = kk < S_.pl ? S_.kbp : S_.kb;                                    \
            const uint16_t *vs_ = kk < S_.pl ? S_.vbp : S_.vb;                                    \
            _Pragma("unroll") for (int c = 0; c < DC; ++c) {                                      \
                kr[i][c] = *reinterpret_cast<const u32x4 *>(ks_ + (int64_t)kk * D + c * 32);      \
                vr[i][c] = *reinterpret_cast<const u32x4 *>(vs_ + (int64_t)kk * D + c * 32);      \
            }                                                                                     \
        }                                                                                         \
    }
    const Seg s_none{0, 0, 0, 0, 0, 0, 0, kA, vA, kA, vA};
    SWH_PAIR_ISSUE(s0, s_none, 0)  // the first segment's KV stream is in flight during RoPE

    // RoPE of both rows' query heads (columns 0 .. 2 GQ - 1) and new keys; new values
    for (int idx = tid; idx < 2 * (GQ + 1) * HD; idx += NT) {
        const int r = idx / ((GQ + 1) * HD), rem = idx - r * (GQ + 1) * HD;
        const int hh = rem / HD, i = rem - hh * HD;
        const int64_t b = r ? bB : bA;
        const int pos = (r ? plB : plA) + step;
        const uint16_t *row = qkv + b * (int64_t)(Hq + 2 * Hkv) * D;
        const float c = rcos[(int64_t)pos * HD + i], s = rsin[(int64_t)pos * HD + i];
        const uint16_t *src = (hh < GQ) ? row + (kvh * GQ + hh) * D : row + (Hq + kvh) * D;
        const float x1 = bf16_bits_to_f32(src[i]), x2 = bf16_bits_to_f32(src[i + HD]);
        const uint16_t o1 = f32_to_bf16_bits(round_bf16(x1 * c) + round_bf16(-x2 * s));
        const uint16_t o2 = f32_to_bf16_bits(round_bf16(x2 * c) + round_bf16(x1 * s));
        if (hh < GQ) {
            q_s[(r * GQ + hh) * D + i] = o1;
            q_s[(r * GQ + hh) * D + i + HD] = o2;
        } else {
            kn_s[r][i] = o1;
            kn_s[r][i + HD] = o2;
        }
    }
    for (int idx = 2 * GQ * D + tid; idx < 16 * D; idx += NT) q_s[idx] = 0;
    for (int d = tid; d < 2 * D; d += NT) {
        const int r = d / D;
        vn_s[r][d - r * D] = qkv[(r ? bB : bA) * (int64_t)(Hq + 2 * Hkv) * D + (Hq + Hkv + kvh) * D + d - r * D];
    }
    lds_barrier();
    for (int d = tid; d < (hasB ? 2 : 1) * D; d += NT) {  // KV append of both rows
        const int r = d / D, e = d - r * D;
        const int64_t cb = r ? cbB : cbA;
        kc[cb + (int64_t)slot_new * D + e] = kn_s[r][e];
        vc[cb + (int64_t)slot_new * D + e] = vn_s[r][e];
    }

    u32x4 qb[DC];
#pragma unroll
    for (int c = 0; c < DC; ++c) qb[c] = *reinterpret_cast<const u32x4 *>(q_s + c16 * D + c * 32 + g * 8);
    float m = kNegInf, l = 0.f;
    f32x4 o[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d) o[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    uint16_t *vt = reinterpret_cast<uint16_t *>(slot_s[wid]);

    bool first = true;
    auto run = [&](const Seg &X, const Seg &Y) __attribute__((always_inline)) {
        const int vlen = (X.hi - X.lo + 15) / 16 * 16 + (Y.hi - Y.lo);
        if (X.hi <= X.lo && Y.hi <= Y.lo) return;
        for (int base = 0; base < vlen; base += KPR) {
            if (!first) {
                SWH_PAIR_ISSUE(X, Y, base)
            }
            first = false;
            f32x4 sc[JB];
            float mx = m;
            bool live[JB];  // block i holds some key (wave-uniform)
#pragma unroll
            for (int i = 0; i < JB; ++i) {
                SWH_PAIR_BLOCK(X, Y, base + (wid + i * NW) * 16, S, k0)
                const bool colv = c16 >= S.clo && c16 < S.chi;  // this lane's column scores these keys
                sc[i] = f32x4{kNegInf, kNegInf, kNegInf, kNegInf};
                live[i] = k0 < S.hi;
                if (k0 < S.hi) {  // wave-uniform
                    const bool fresh = S.fresh && (k0 + c16 == S.n - 1);  // the new key/value, from LDS
                    const int fr = S.fresh == 2 ? 1 : 0;
#pragma unroll
                    for (int c = 0; c < DC; ++c) {
                        const u32x4 kn = *reinterpret_cast<const u32x4 *>(kn_s[fr] + c * 32 + g * 8);
                        const u32x4 vn = *reinterpret_cast<const u32x4 *>(vn_s[fr] + c * 32 + g * 8);
                        kr[i][c] = fresh ? kn : kr[i][c];
                        vr[i][c] = fresh ? vn : vr[i][c];
                    }
                    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int c = 0; c < DC; ++c)
                        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kr[i][c]),
                                                                      __builtin_bit_cast(bf16x8, qb[c]), acc, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        sc[i][r] = (colv && k0 + 4 * g + r < S.hi) ? acc[r] * scale : kNegInf;
                        mx = fmaxf(mx, sc[i][r]);
                    }
                }
            }
            mx = fmaxf(mx, __shfl_xor(mx, 16, kWave));
            mx = fmaxf(mx, __shfl_xor(mx, 32, kWave));
            const float corr = (mx == kNegInf) ? 1.f : expf(m - mx);
            l *= corr;
#pragma unroll
            for (int d = 0; d < DB; ++d) o[d] *= corr;
            m = mx;
#pragma unroll
            for (int i = 0; i < JB; i += 2) {
                if (live[i] || live[i + 1]) {  // wave-uniform
                    float pj[8];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        pj[r] = (mx == kNegInf) ? 0.f : expf(sc[i][r] - mx);
                        pj[4 + r] = (mx == kNegInf) ? 0.f : expf(sc[i + 1][r] - mx);
                        l += pj[r] + pj[4 + r];
                    }
#pragma unroll
                    for (int c = 0; c < DC; ++c) {
                        *reinterpret_cast<u32x4 *>(vt + c16 * VS + c * 32 + g * 8) =
                            live[i] ? vr[i][c] : u32x4{0u, 0u, 0u, 0u};
                        *reinterpret_cast<u32x4 *>(vt + (16 + c16) * VS + c * 32 + g * 8) =
                            live[i + 1] ? vr[i + 1][c] : u32x4{0u, 0u, 0u, 0u};
                    }
                    uint32_t pb[4];
#pragma unroll
                    for (int h = 0; h < 4; ++h)
                        pb[h] = __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{pj[2 * h], pj[2 * h + 1]}, bf16x2));
                    const bf16x8 pbf = __builtin_bit_cast(bf16x8, u32x4{pb[0], pb[1], pb[2], pb[3]});
                    const int q = c16 >> 2, pq = c16 & 3;
#pragma unroll
                    for (int d = 0; d < DB; ++d) {
                        const bf16x4s lo = lds_read_tr16(vt + (4 * g + q) * VS + d * 16 + 4 * pq);
                        const bf16x4s hi = lds_read_tr16(vt + (16 + 4 * g + q) * VS + d * 16 + 4 * pq);
                        const bf16x8 va = __builtin_bit_cast(
                            bf16x8, u32x4{__builtin_bit_cast(uint2, lo).x, __builtin_bit_cast(uint2, lo).y,
                                          __builtin_bit_cast(uint2, hi).x, __builtin_bit_cast(uint2, hi).y});
                        o[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pbf, o[d], 0, 0, 0);
                    }
                }
            }
        }
    };
    run(s0, s_none);
    first = false;  // s0 may be empty (a zero-length prompt): the next run issues its own first round
    if (!shared) run(sBp, s_none);
    run(sAo, sBo);  // both rows' own keys: A's blocks, then B's, sharing rounds
#undef SWH_PAIR_ISSUE
#undef SWH_PAIR_BLOCK
    l += __shfl_xor(l, 16, kWave);
    l += __shfl_xor(l, 32, kWave);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    float *rec = red_s(wid, c16);
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int r = 0; r < 4; ++r) rec[d * 16 + 4 * g + r] = o[d][r];
    if (g == 0) {
        rec[D] = m;
        rec[D + 1] = l;
    }
    __syncthreads();
    auto merged = [&](int h, int d) -> uint16_t {  // the waves' (m, l, acc) of column h, dim d
        float mxw = kNegInf;
#pragma unroll
        for (int w2 = 0; w2 < NW; ++w2) mxw = fmaxf(mxw, red_s(w2, h)[D]);
        float Ls = 0.f, A = 0.f;
#pragma unroll
        for (int w2 = 0; w2 < NW; ++w2) {
            const float *rw = red_s(w2, h);
            const float mq = rw[D];
            if (mq == kNegInf) continue;
            const float cq = expf(mq - mxw);
            Ls = fmaf(rw[D + 1], cq, Ls);
            A = fmaf(rw[d], cq, A);
        }
        return f32_to_bf16_bits(A / Ls);
    };
    const int nrow = hasB ? 2 : 1;
    if (pf.ofrag) {
        for (int idx = tid; idx < nrow * GQ * D; idx += NT) {  // GQ * D % 64 == 0: whole waves per row
            const int h = idx / D, d = idx - h * D, r = h / GQ;
            const uint32_t v = merged(h, d);
            const uint32_t p2 = v | (__shfl_down(v, 1, kWave) << 16);
            const uint32_t p4 = __shfl_down(p2, 2, kWave);
            const uint32_t p6 = __shfl_down(p2, 4, kWave), p8 = __shfl_down(p2, 6, kWave);
            if ((lane & 7) == 0)
                *reinterpret_cast<uint4 *>(out + frag_at(bA + r, (kvh * GQ + h - r * GQ) * D + d, Hq * D)) =
                    uint4{p2, p4, p6, p8};
        }
    } else {
        for (int idx = tid; idx < nrow * GQ * D; idx += NT) {
            const int h = idx / D, d = idx - h * D, r = h / GQ;
            out[(bA + r) * (int64_t)Hq * D + (kvh * GQ + h - r * GQ) * D + d] = merged(h, d);
        }
    }
}

template <int D, int GQ>
int launch_attn(const uint16_t *q, uint16_t *kc, uint16_t *vc, const float *rc, const float *rs, const int32_t *pl,
                const int32_t *st, int64_t B, int Hq, int Hkv, int Tmax, float scale, uint16_t *o, hipStream_t s,
                const AttnPrefetch &pf) {
    // warm-up rows: whole grid rows of Hkv workgroups
    int64_t extra = 0;
    if (pf.jobs) {
        extra = (pf.nwg + Hkv - 1) / Hkv;
        if (B + extra > 65535) extra = 0;
    }
    if constexpr (D == 128 && 2 * GQ <= 16) {
        if (launch_policy().attn_pair) {  // row pairs: (B + 1) / 2 grid rows, then the warm-up rows
            const int64_t pairs = (B + 1) / 2;
            if (pairs + extra > 65535) extra = 0;
            attn_decode_pair_kernel<D, GQ><<<dim3((unsigned)Hkv, (unsigned)(pairs + extra)), 512, 0, s>>>(
                q, kc, vc, rc, rs, pl, st, Hq, Hkv, Tmax, scale, o, pf);
            return launch_status();
        }
    }
    attn_decode_kernel<D, GQ><<<dim3((unsigned)Hkv, (unsigned)(B + extra)), attn_threads(D), 0, s>>>(
        q, kc, vc, rc, rs, pl, st, Hq, Hkv, Tmax, scale, o, pf);
    return launch_status();
}

template <int D>
int attn_dispatch_gq(int gq, const uint16_t *q, uint16_t *kc, uint16_t *vc, const float *rc, const float *rs,
                     const int32_t *pl, const int32_t *st, int64_t B, int Hq, int Hkv, int Tmax, float scale,
                     uint16_t *o, hipStream_t s, const AttnPrefetch &pf) {
    switch (gq) {
    case 1: return launch_attn<D, 1>(q, kc, vc, rc, rs, pl, st, B, Hq, Hkv, Tmax, scale, o, s, pf);
    case 2: return launch_attn<D, 2>(q, kc, vc, rc, rs, pl, st, B, Hq, Hkv, Tmax, scale, o, s, pf);
    case 3: return launch_attn<D, 3>(q, kc, vc, rc, rs, pl, st, B, Hq, Hkv, Tmax, scale, o, s, pf);
    case 4: return launch_attn<D, 4>(q, kc, vc, rc, rs, pl, st, B, Hq, Hkv, Tmax, scale, o, s, pf);
    case 5: return launch_attn<D, 5>(q, kc, vc, rc, rs, pl, st, B, Hq, Hkv, Tmax, scale, o, s, pf);
    case 6: return launch_attn<D, 6>(q, kc, vc, rc, rs, pl, st, B, Hq, Hkv, Tmax, scale, o, s, pf);
    case 7: return launch_attn<D, 7>(q, kc, vc, rc, rs, pl, st, B, Hq, Hkv, Tmax, scale, o, s, pf);
    case 8: return launch_attn<D, 8>(q, kc, vc, rc, rs, pl, st, B, Hq, Hkv, Tmax, scale, o, s, pf);
    default: return SWH_E_ARG;
    }
}

}  // namespace
}  // namespace swh

using namespace swh;

static int attn_decode_impl(const void *qkv, void *k_cache, void *v_cache, const float *rope_cos,
                            const float *rope_sin, const int32_t *prompt_len, const int32_t *prompt_row,
                            const int32_t *state, int64_t B, int32_t Hq, int32_t Hkv, int32_t D, int32_t Tmax,
                            float scale, void *out, int32_t out_frag, AttnPrefetch pf, void *stream) {
    if (!qkv || !k_cache || !v_cache || !rope_cos || !rope_sin || !prompt_len || !state || !out || B < 0 || Hkv <= 0 ||
        Hq % Hkv || Tmax <= 0 || B > 65535 || (out_frag & ~1))
        return SWH_E_ARG;
    if (out_frag && (B % 16 || (Hq * D) % 32 || (reinterpret_cast<uintptr_t>(out) & 15))) return SWH_E_ARG;
    if (B == 0) return SWH_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const auto *q = static_cast<const uint16_t *>(qkv);
    auto *kc = static_cast<uint16_t *>(k_cache), *vc = static_cast<uint16_t *>(v_cache);
    auto *o = static_cast<uint16_t *>(out);
    const int gq = Hq / Hkv;
    pf.rows = (int)B;
    pf.prow = prompt_row;
    pf.ofrag = out_frag;
    if (D == 64) return attn_dispatch_gq<64>(gq, q, kc, vc, rope_cos, rope_sin, prompt_len, state, B, Hq, Hkv, Tmax, scale, o, s, pf);
    if (D == 128) return attn_dispatch_gq<128>(gq, q, kc, vc, rope_cos, rope_sin, prompt_len, state, B, Hq, Hkv, Tmax, scale, o, s, pf);
    return SWH_E_ARG;
}

extern "C" int swh_attn_decode_shared_frag(const void *qkv, void *k_cache, void *v_cache, const float *rope_cos,
                                           const float *rope_sin, const int32_t *prompt_len,
                                           const int32_t *prompt_row, const int32_t *state, int64_t B, int32_t Hq,
                                           int32_t Hkv, int32_t D, int32_t Tmax, float scale, void *out,
                                           int32_t out_frag, void *stream) {
    return attn_decode_impl(qkv, k_cache, v_cache, rope_cos, rope_sin, prompt_len, prompt_row, state, B, Hq, Hkv, D,
                            Tmax, scale, out, out_frag, AttnPrefetch{}, stream);
}
// swh_attn_decode_shared_frag whose launch also carries Infinity Cache warm-up
// workgroups (on the CUs the attention leaves idle) over l3_jobs
extern "C" int swh_attn_decode_l3(const void *qkv, void *k_cache, void *v_cache, const float *rope_cos,
                                  const float *rope_sin, const int32_t *prompt_len, const int32_t *prompt_row,
                                  const int32_t *state, int64_t B, int32_t Hq, int32_t Hkv, int32_t D, int32_t Tmax,
                                  float scale, void *out, int32_t out_frag, const void *l3_jobs, int32_t l3_njobs,
                                  int32_t l3_wgs, void *l3_sink, void *stream) {
    if (!l3_jobs || !l3_sink || l3_njobs <= 0 || l3_njobs > kL3MaxJobs || l3_wgs <= 0 || l3_wgs > 4096 || Hkv <= 0)
        return SWH_E_ARG;
    AttnPrefetch pf{};
    pf.jobs = static_cast<const L3Job *>(l3_jobs);
    pf.njobs = l3_njobs;
    pf.sink = static_cast<uint32_t *>(l3_sink);
    // the sink holds one word per thread of every warm-up workgroup (whole grid rows)
    pf.nwg = (l3_wgs + Hkv - 1) / Hkv * Hkv;
    return attn_decode_impl(qkv, k_cache, v_cache, rope_cos, rope_sin, prompt_len, prompt_row, state, B, Hq, Hkv, D,
                            Tmax, scale, out, out_frag, pf, stream);
}

extern "C" int swh_attn_decode_shared(const void *qkv, void *k_cache, void *v_cache, const float *rope_cos,
                                      const float *rope_sin, const int32_t *prompt_len, const int32_t *prompt_row,
                                      const int32_t *state, int64_t B, int32_t Hq, int32_t Hkv, int32_t D, int32_t Tmax,
                                      float scale, void *out, void *stream) {
    return swh_attn_decode_shared_frag(qkv, k_cache, v_cache, rope_cos, rope_sin, prompt_len, prompt_row, state, B, Hq,
                                       Hkv, D, Tmax, scale, out, 0, stream);
}

extern "C" int swh_attn_decode(const void *qkv, void *k_cache, void *v_cache, const float *rope_cos,
                               const float *rope_sin, const int32_t *prompt_len, const int32_t *state, int64_t B,
                               int32_t Hq, int32_t Hkv, int32_t D, int32_t Tmax, float scale, void *out,
                               void *stream) {
    return swh_attn_decode_shared(qkv, k_cache, v_cache, rope_cos, rope_sin, prompt_len, nullptr, state, B, Hq, Hkv, D,
                                  Tmax, scale, out, stream);
}
