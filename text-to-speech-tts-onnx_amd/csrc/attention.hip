// attention.hip — flash-style attention for the DiT blocks on gfx950 MFMA.
//
// Reference: AttnProcessor.__call__ (F5_TTS/modeling_modified/F5/modules.py:467):
//     softmax(q @ k, dim=-1, dtype=float32) @ v      — no mask, no 1/sqrt(d) (folded into W_q, W_k).
// The reference materialises the (2,16,N,N) logits; here K/V stream through LDS in 64-key stages and
// the softmax is online (running max / sum in fp32), so HBM traffic is q,k,v,o only.
//
// Tiling (wave64, 32x32 MFMA tiles, head_dim = 64):
//   workgroup = 4 waves = 128 queries of one (batch, head); each wave owns 32 queries.
//   S^T = K Q^T   (rows = keys, cols = queries): lane l holds query (l&31) and 16 of the 32 keys
//                 [key kappa(r) = (r&3) + 8*(r>>2) + 4*(l>>5)], so a query's softmax statistics are
//                 per-lane: 16 in-register values + ONE cross-lane exchange with lane^32.
//   O^T = V^T P^T (rows = head-dim, cols = queries): the probabilities a lane holds are already in the
//                 MFMA B-operand position (k = key, j = query) — keys are simply consumed in kappa
//                 order, and V is fetched in that same order — no LDS round trip for P, and the
//                 rescale factor exp(m_old - m_new) is again per-lane.
//   fp32 : v_mfma_f32_32x32x2_f32 (exact fp32 products, K = 2 keys per instruction)
//   f16/bf16 : v_mfma_f32_32x32x16 — V is staged transposed ([d][key]) so that the 8 keys a lane feeds
//                 per instruction are two contiguous 8-byte LDS reads.
// Host side (end of this file): attention_plan() decides the K / V layout the QKV epilogue writes together with the kernel form, the
// grid and the key slices, once per evaluation; launch_attention() looks the plan's form up in one dispatch table and launches.
#include "common.h"
#include <functional>
#include <map>
#include <mutex>
#include <tuple>
#include "mfma.h"
#include "f5_kernels.h"
#include "x3_split.h"
#include "lds_dma.h"         // lds_addr, wait_vm, wait_lgkm, buf_rsrc
#include <type_traits>
#include <string>
#include <algorithm>

namespace mi {

// SPLIT2 = false: workgroup = 4 waves x 32 queries, every wave walks all keys.
// SPLIT2 = true : workgroup = 2 x 32 queries; waves (2g, 2g+1) share query group g and take the even / odd 32-key tile of
//                 every 64-key stage, then wave 2g+1 hands its (max, sum, O) to wave 2g through LDS.  Twice as many, half
//                 as long workgroups: the fp32 kernel is MFMA-bound, and one utterance is 9 x 32 = 288 workgroups on 256
//                 CUs, so the CUs that got two workgroups set the makespan (2 units); 576 half-size ones finish in 1.5.
// X3S (fp32 only): the S^T = K Q^T products as exact three-way bf16 splits on the bf16 pipes (gemm_x3.hip has the
//                 arithmetic): 24 v_mfma_f32_32x32x16_bf16 (768 cycles) instead of 32 v_mfma_f32_32x32x2_f32 (2048) per 32x32
//                 tile; Q is split once per workgroup, the K fragments on their way from LDS (176 VALU instructions per
//                 tile, overlapped by the co-resident waves).  P V stays on the native fp32 MFMA (it wants V transposed).
// REFH (f16 only): the rounding points of the reference's fp16-transformer export (F5/fp16/modules.py:467, Export_F5.py:321-326):
//                 q / k carry an extra x0.1 each (folded into the projections before they are rounded to fp16), the scores
//                 leave the q k product as fp16 values, are widened and multiplied by `sscale` (= 100) in fp32, softmax in fp32,
//                 probabilities rounded to fp16 for P V.  Q is therefore NOT pre-multiplied by log2(e) (that would re-round
//                 it): log2(e) rides on `sscale`.
// Workgroup -> (query tile, head).  Consecutive workgroup ids (x fastest) go to consecutive XCDs, so the query tiles of one head
// — which all stream that head's K and V — land on up to eight different L2s and each fetches K / V from the fabric for itself.
// With `xmap` (heads a multiple of 8) the ids are re-read so that XCD x serves heads x, x + 8, ...: a head's query tiles share
// one L2.  Each z plane (key slice) starts at XCD 0 because gridDim.x * gridDim.y is then a multiple of 8.
#define ATTN_XCD_MAP                                                                          \
    int bx_ = (int)blockIdx.x, by_ = (int)blockIdx.y;                                         \
    if (xmap) {                                                                               \
        const int l2 = bx_ + (int)gridDim.x * by_, slot = l2 >> 3;                            \
        by_ = (l2 & 7) + 8 * (slot / (int)gridDim.x);                                         \
        bx_ = slot % (int)gridDim.x;                                                          \
    }

// VARLEN (ragged F5 batches, padded slabs): item b = bh / H holds NL = lens[b / 2] live rows of its N (the CFG pair 2u, 2u + 1
// shares utterance u's length); N stays the row stride of q / k / v / o, NL replaces it in every mask and loop bound.
//   * keys >= NL are masked exactly like keys >= N: score -inf, their V^T values cleared before the P V product;
//   * query rows in [NL, N) are stored as zeros (o and o_planes);
//   * a query tile whose first row is >= NL is `dead`: it loads no stage; slice z = 0 stores its zero rows, the other
//     slices return at once.  Every slice of a dead tile skips the merge, so no ticket of `cnt` is taken for it;
//   * a live tile runs every slice and every slice takes its ticket.  A slice whose stages lie wholly past NL (st0 >= nstage
//     after the clamp to ceil(NL / 64)) publishes the neutral partial m = -inf, l = 0, O = 0 — the empty slices attn_z_force
//     makes — and the merge weighs it by 0 (the m == -inf test: no exp(-inf - (-inf))).  At least one slice of a live tile
//     holds stage 0, so the merged l is > 0.  The last arriver resets the counter, so a completed launch leaves every
//     counter at 0 for whatever length mix the next replay brings.
// VARLEN = false: NL = N and dead = false are constants, the instantiations compile to the code they had without the switch.
#define ATTN_VARLEN_PROLOGUE                                                                  \
    const int NL = VARLEN ? lens[(bh / H) >> 1] : N;                                          \
    const bool dead = VARLEN && (SPLIT2 ? bx_ * 64 : bx_ * 128) >= NL;                        \
    if (dead && blockIdx.z != 0) return;

// lane <-> lane ^ 32 exchange of the online softmax (row max, row sum: a query column lives in lanes l and l + 32) on
// v_permlane32_swap instead of ds_bpermute (no LDS-crossbar round trip on the S -> max -> exp chain).  Two copies of the value
// go in; the instruction leaves {own low | low} in one register and {high | own high} in the other, so their max / sum is the
// pair's in every lane, and a + b == b + a bit for bit: both halves still agree and the values are those of the shuffle form.
// Inline asm: on this toolchain the builtin returns the first register twice (tools/ubench/permlane32b.hip); the s_nop covers
// the VALU-write -> permlane-read hazard (two wait states).
__device__ __forceinline__ void xor32_pair(float v, float& a, float& b) {
    a = v; b = v;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ float xor32_max(float v) { float a, b; xor32_pair(v, a, b); return fmaxf(a, b); }
__device__ __forceinline__ float xor32_sum(float v) { float a, b; xor32_pair(v, a, b); return a + b; }

template <typename T, bool SPLIT2 = false, bool X3S = false, bool REFH = false, bool VARLEN = false>
__global__ __launch_bounds__(256, 3) void attn_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                   const T* __restrict__ v, T* __restrict__ o, int H, int N,
                                                   float* __restrict__ ws, int* __restrict__ cnt, float sscale = 1.f, int xmap = 0,
                                                   const int* __restrict__ lens = nullptr) {
    static_assert(!REFH || (sizeof(T) == 2 && !X3S), "REFH is the fp16 form");
    ATTN_XCD_MAP
    using MF = Mfma<T>;
    constexpr int KP = MF::KP;
    constexpr int D = 64, KT = 64;
    constexpr int VEC = 16 / (int)sizeof(T);
    constexpr int KS = D / (2 * KP);                       // MFMA k-steps over head_dim for S^T
    static_assert(!X3S || sizeof(T) == 4, "the split form is the fp32 kernel");
    constexpr int LDK = D + (sizeof(T) == 4 ? (X3S ? 4 : 1) : 8);         // X3S: 16-byte aligned rows (float4 fragment reads)
    constexpr int LDV = sizeof(T) == 4 ? D : KT + 4;       // fp32: Vs[key][d] ; 16-bit: Vt[d][key]
    constexpr int NV = KT * D / VEC / 256;                 // 16-byte vectors per thread per tile
    __shared__ __attribute__((aligned(16))) T smem[KT * LDK + (sizeof(T) == 4 ? KT * D : D * LDV)];
    T* Ks = smem;
    T* Vs = smem + KT * LDK;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 31, hi = lane >> 5;
    const int bh = by_;
    ATTN_VARLEN_PROLOGUE
    if constexpr (VARLEN) {
        if (dead) {          // slice 0 of a tile with no live query: its rows leave as zeros, and nothing below runs (no ticket)
            const int r0 = SPLIT2 ? bx_ * 64 : bx_ * 128, r1 = min(r0 + (SPLIT2 ? 64 : 128), N);
            constexpr int VPR = D * (int)sizeof(T) / 16;                // 16-byte vectors per row of one head
            const int b = bh / H, h = bh - b * H;
            for (int i = tid; i < (r1 - r0) * VPR; i += 256)
                *reinterpret_cast<uint4*>(o + ((long)b * N + r0 + i / VPR) * H * D + h * D + (i % VPR) * (16 / (int)sizeof(T))) = make_uint4(0, 0, 0, 0);
            return;
        }
    }
    const int q0 = SPLIT2 ? bx_ * 64 + (wave >> 1) * 32 : bx_ * 128 + wave * 32;
    const T* qb = q + (long)bh * N * D;
    const T* kb = k + (long)bh * N * D;
    const long vld = sizeof(T) == 4 ? 0 : (long)((N + 7) / 8 * 8);
    const T* vb = v + (sizeof(T) == 4 ? (long)bh * N * D : (long)bh * D * vld);

    // ---- Q fragments (B operand of S^T): Q[q = q0+lr][d = ks*2KP + hi*KP ..] ------------------
    typename MF::Frag qf[X3S ? 1 : KS];
    bf16x8 qf3[X3S ? 4 : 1][3];                            // X3S: Q[q][16 ks + 8 hi .. +8] as three bf16 pieces, pre-scaled by log2(e)
    if constexpr (X3S) {
        const int qr = q0 + lr;
        const bool ok = qr < NL;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            float4 a = float4{0.f, 0.f, 0.f, 0.f}, b = a;
            if (ok) {
                a = *reinterpret_cast<const float4*>(qb + (long)qr * D + ks * 16 + hi * 8);
                b = *reinterpret_cast<const float4*>(qb + (long)qr * D + ks * 16 + hi * 8 + 4);
            }
            constexpr float L2E = 1.4426950408889634f;
            unsigned u1[4], u2[4], u3[4];
            x3_split_pair(a.x * L2E, a.y * L2E, u1[0], u2[0], u3[0]);
            x3_split_pair(a.z * L2E, a.w * L2E, u1[1], u2[1], u3[1]);
            x3_split_pair(b.x * L2E, b.y * L2E, u1[2], u2[2], u3[2]);
            x3_split_pair(b.z * L2E, b.w * L2E, u1[3], u2[3], u3[3]);
            qf3[ks][0] = __builtin_bit_cast(bf16x8, u32x4{u1[0], u1[1], u1[2], u1[3]});
            qf3[ks][1] = __builtin_bit_cast(bf16x8, u32x4{u2[0], u2[1], u2[2], u2[3]});
            qf3[ks][2] = __builtin_bit_cast(bf16x8, u32x4{u3[0], u3[1], u3[2], u3[3]});
        }
    } else {
        const int qr = q0 + lr;
        const bool ok = qr < NL;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            // Q is pre-multiplied by log2(e): the softmax then needs v_exp_f32 (2^x) only, no expf expansion
            if constexpr (KP == 1) {
                qf[ks] = ok ? qb[(long)qr * D + 2 * ks + hi] * 1.4426950408889634f : 0.f;
            } else {
                uint4 raw = make_uint4(0, 0, 0, 0);
                if (ok) raw = *reinterpret_cast<const uint4*>(qb + (long)qr * D + ks * 16 + hi * 8);
                T* e = reinterpret_cast<T*>(&raw);
#pragma unroll
                for (int j = 0; j < 8; ++j) if constexpr (!REFH) e[j] = from_f32<T>(to_f32(e[j]) * 1.4426950408889634f);
                qf[ks] = *reinterpret_cast<const typename MF::Frag*>(&raw);
            }
        }
    }

    uint4 kreg[NV], vreg[NV];
    auto load_regs = [&](int key0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int vi = tid + i * 256;
            const int key = vi / (D / VEC), dv = vi - key * (D / VEC);
            uint4 a = make_uint4(0, 0, 0, 0), b = make_uint4(0, 0, 0, 0);
            if (key0 + key < NL) a = *reinterpret_cast<const uint4*>(kb + (long)(key0 + key) * D + dv * VEC);
            if constexpr (sizeof(T) == 4) {
                if (key0 + key < NL) b = *reinterpret_cast<const uint4*>(vb + (long)(key0 + key) * D + dv * VEC);
            } else {
                // V arrives transposed from the QKV epilogue: row d = vi / 8, eight consecutive keys per vector
                const int d = vi >> 3, kv = vi & 7;
                if (key0 + kv * 8 < NL) b = *reinterpret_cast<const uint4*>(vb + (long)d * vld + key0 + kv * 8);
                if constexpr (VARLEN) {       // keys [NL, N) are padding rows of the slab: clear their V^T values (16-bit halves)
                    const int keep = NL - (key0 + kv * 8);
                    if (keep > 0 && keep < 8) {
                        unsigned w[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) w[e] &= (2 * e < keep ? 0x0000ffffu : 0u) | (2 * e + 1 < keep ? 0xffff0000u : 0u);
                        b = make_uint4(w[0], w[1], w[2], w[3]);
                    }
                }
            }
            kreg[i] = a; vreg[i] = b;
        }
    };
    auto store_lds = [&]() {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int vi = tid + i * 256;
            const int key = vi / (D / VEC), dv = vi - key * (D / VEC);
            if constexpr (sizeof(T) == 4) {
                float* d = reinterpret_cast<float*>(Ks) + key * LDK + dv * VEC;
                d[0] = __uint_as_float(kreg[i].x); d[1] = __uint_as_float(kreg[i].y);
                d[2] = __uint_as_float(kreg[i].z); d[3] = __uint_as_float(kreg[i].w);
                *reinterpret_cast<uint4*>(Vs + key * LDV + dv * VEC) = vreg[i];
            } else {
                *reinterpret_cast<uint4*>(Ks + key * LDK + dv * VEC) = kreg[i];
                const int d = vi >> 3, kv = vi & 7;                                           // Vt[d][key], 8-byte aligned rows
                *reinterpret_cast<uint2*>(Vs + d * LDV + kv * 8) = make_uint2(vreg[i].x, vreg[i].y);
                *reinterpret_cast<uint2*>(Vs + d * LDV + kv * 8 + 4) = make_uint2(vreg[i].z, vreg[i].w);
            }
        }
    };

    f32x16 oacc[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { oacc[0][r] = 0.f; oacc[1][r] = 0.f; }
    float m_run = -INFINITY, l_run = 0.f;

    // gridDim.z > 1 (SPLIT2 only): the 64-key stages are cut into gridDim.z contiguous slices, one workgroup each; the
    // slices of a query tile meet in `ws` and the LAST one to arrive merges them in slice order (see the end of the kernel)
    const int nstage_all = (NL + KT - 1) / KT;
    const int st0 = SPLIT2 ? (int)((long)blockIdx.z * nstage_all / gridDim.z) : 0;
    const int nstage = SPLIT2 ? (int)((long)(blockIdx.z + 1) * nstage_all / gridDim.z) : nstage_all;
    if (st0 < nstage) {
        load_regs(st0 * KT);
        store_lds();
        __syncthreads();
    }
    for (int st = st0; st < nstage; ++st) {
        if (st + 1 < nstage) load_regs((st + 1) * KT);
        auto tile = [&](int kt) {                                        // one 32-key tile
            const int key0 = st * KT + kt * 32;
            // ---- S^T tile: 32 keys x 32 queries ----------------------------------------------
            f32x16 sacc;
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
            if constexpr (X3S) {
                const float* krow = reinterpret_cast<const float*>(Ks) + (kt * 32 + lr) * LDK + hi * 8;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const float4 a = *reinterpret_cast<const float4*>(krow + ks * 16), b = *reinterpret_cast<const float4*>(krow + ks * 16 + 4);
                    unsigned u1[4], u2[4], u3[4];
                    x3_split_pair(a.x, a.y, u1[0], u2[0], u3[0]);
                    x3_split_pair(a.z, a.w, u1[1], u2[1], u3[1]);
                    x3_split_pair(b.x, b.y, u1[2], u2[2], u3[2]);
                    x3_split_pair(b.z, b.w, u1[3], u2[3], u3[3]);
                    const bf16x8 k1 = __builtin_bit_cast(bf16x8, u32x4{u1[0], u1[1], u1[2], u1[3]});
                    const bf16x8 k2 = __builtin_bit_cast(bf16x8, u32x4{u2[0], u2[1], u2[2], u2[3]});
                    const bf16x8 k3 = __builtin_bit_cast(bf16x8, u32x4{u3[0], u3[1], u3[2], u3[3]});
                    // six partial products, small terms first
                    sacc = Mfma<bf16>::mma(k1, qf3[ks][2], sacc);
                    sacc = Mfma<bf16>::mma(k2, qf3[ks][1], sacc);
                    sacc = Mfma<bf16>::mma(k3, qf3[ks][0], sacc);
                    sacc = Mfma<bf16>::mma(k1, qf3[ks][1], sacc);
                    sacc = Mfma<bf16>::mma(k2, qf3[ks][0], sacc);
                    sacc = Mfma<bf16>::mma(k1, qf3[ks][0], sacc);
                }
            } else {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const typename MF::Frag a =
                        *reinterpret_cast<const typename MF::Frag*>(Ks + (kt * 32 + lr) * LDK + ks * 2 * KP + hi * KP);
                    sacc = MF::mma(a, qf[ks], sacc);
                }
            }
            if constexpr (REFH) {
                // torch.matmul(query, key) is an fp16 tensor; `.float() * 100.0` follows (fp16/modules.py:467)
                const float c = sscale * 1.4426950408889634f;
#pragma unroll
                for (int r = 0; r < 16; ++r) sacc[r] = to_f32(from_f32<T>(sacc[r])) * c;
            }
            // ---- online softmax (per lane = per query) -----------------------------------------
            // only the tile that straddles N needs the key >= N select (2 VALU issues per score, a third of the
            // softmax's VALU time when done on every tile): wave-uniform branch around it
            if (key0 + 32 > NL) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = key0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    if (key >= NL) sacc[r] = -INFINITY;
                }
            }
            float mloc = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) mloc = fmaxf(mloc, sacc[r]);
            mloc = fmaxf(mloc, __shfl_xor(mloc, 32));         // (v_permlane32_swap measured 1 % SLOWER in this kernel, 3.5 % faster in attn_x3f_kernel)
            // lazy rescale: keep the old reference max while it is within 2^8 of the new one (P <= 256, exact in
            // fp32 accumulation); rescale O and l only when some query of the wave needs it (wave-uniform branch)
            float alpha = 1.f;
            if (!__all(mloc - m_run <= 8.0f)) {
                const float m_new = fmaxf(m_run, mloc);
                alpha = __builtin_amdgcn_exp2f(m_run - m_new);
                m_run = m_new;
#pragma unroll
                for (int r = 0; r < 16; ++r) { oacc[0][r] *= alpha; oacc[1][r] *= alpha; }
            }
            // score - max and the row sum as packed fp32 pairs (v_pk_add_f32: two per VALU issue)
            typedef float f2 __attribute__((ext_vector_type(2)));
            float p[16];
            f2 ls2 = f2{0.f, 0.f};
            const f2 m2 = f2{m_run, m_run};
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const f2 d = f2{sacc[r], sacc[r + 1]} - m2;
                const f2 e = f2{__builtin_amdgcn_exp2f(d.x), __builtin_amdgcn_exp2f(d.y)};
                p[r] = e.x; p[r + 1] = e.y;
                ls2 += e;
            }
            float lsum = ls2.x + ls2.y;
            lsum += __shfl_xor(lsum, 32);
            l_run = l_run * alpha + lsum;
            // ---- O^T += V^T P^T ------------------------------------------------------------------
            if constexpr (KP == 1) {
#pragma unroll
                for (int s = 0; s < 16; ++s) {
                    const int kk = kt * 32 + (s & 3) + 8 * (s >> 2) + 4 * hi;
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt)
                        oacc[dt] = MF::mma(reinterpret_cast<const float*>(Vs)[kk * LDV + dt * 32 + lr], p[s], oacc[dt]);
                }
            } else {
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    T pb[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) pb[e] = from_f32<T>(p[8 * s2 + e]);
                    const typename MF::Frag bfrag = *reinterpret_cast<const typename MF::Frag*>(pb);
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt) {
                        const T* row = Vs + (dt * 32 + lr) * LDV + kt * 32 + 16 * s2 + 4 * hi;
                        uint2 a2[2];
                        a2[0] = *reinterpret_cast<const uint2*>(row);
                        a2[1] = *reinterpret_cast<const uint2*>(row + 8);
                        oacc[dt] = MF::mma(*reinterpret_cast<const typename MF::Frag*>(a2), bfrag, oacc[dt]);
                    }
                }
            }
        };
        if constexpr (SPLIT2) {
            if (st * KT + (wave & 1) * 32 < NL) tile(wave & 1);           // this wave's half of the stage
        } else {
#pragma unroll
            for (int kt = 0; kt < KT / 32; ++kt) {
                const int key0 = st * KT + kt * 32;
                if (key0 < NL) tile(kt);                                  // wave-uniform
            }
        }
        __syncthreads();
        if (st + 1 < nstage) {
            store_lds();
            __syncthreads();
        }
    }

    bool owner = true;                                              // this wave holds a finished 32-query result
    if constexpr (SPLIT2) {
        // ---- merge the two key halves: m = max(m0, m1) ; l = l0 2^(m0-m) + l1 2^(m1-m) ; O likewise ----------------------
        __syncthreads();                                            // every wave is done with the K / V stage
        float* comb = reinterpret_cast<float*>(smem);               // [2 groups][32 accumulator registers][64 lanes]
        float* stats = comb + 2 * 32 * 64;                          // [2 groups][64 lanes][m, l]
        static_assert(sizeof(smem) >= (2 * 32 * 64 + 2 * 64 * 2 + 4) * sizeof(float), "merge buffer fits the stage");
        const int grp = wave >> 1;
        owner = !(wave & 1);
        if (!owner) {
            stats[(grp * 64 + lane) * 2] = m_run; stats[(grp * 64 + lane) * 2 + 1] = l_run;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) comb[((grp * 2 + dt) * 16 + r) * 64 + lane] = oacc[dt][r];
        }
        __syncthreads();
        if (owner) {
            const float m1 = stats[(grp * 64 + lane) * 2], l1 = stats[(grp * 64 + lane) * 2 + 1];
            const float m = fmaxf(m_run, m1);
            const float s0 = m_run == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m_run - m);
            const float s1 = m1 == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m1 - m);
            l_run = l_run * s0 + l1 * s1;
            m_run = m;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[dt][r] = oacc[dt][r] * s0 + comb[((grp * 2 + dt) * 16 + r) * 64 + lane] * s1;
        }
        // ---- key slices (gridDim.z > 1).  One utterance in fp32 is 18 x 32 = 576 of these workgroups on 768 slots (three per
        // CU): 2.25 per CU, so the CUs that got three set the makespan and a quarter of the chip idles.  With Z slices the
        // work comes in pieces of 1 / Z (Z = 4: exactly 9 per CU).  Every slice publishes (m, l, O) of its keys with
        // write-through stores, drains them, and takes a ticket (relaxed agent-scope fetch-add: the gemm_sk.hip hand-off);
        // the workgroup that draws the last ticket adds the slices IN SLICE ORDER (its own from registers), so the result
        // does not depend on which one that is, resets the ticket counter (hipGraph replays find it at zero) and stores.
        // Nobody waits for anybody: there is no residency requirement. ---------------------------------------------------
        const int Z = (int)gridDim.z;
        if (Z > 1) {
            const int z = (int)blockIdx.z;
            const int unit = (int)(by_ * gridDim.x + bx_);
            constexpr int SLOT = 2 * 32 * 64 + 2 * 64 * 2;           // floats per (unit, slice)
            // write-through (sc1) stores / sc1 loads through a buffer descriptor, as in gemm_sk.hip: no L2-wide write-back fence
            typedef unsigned int u2 __attribute__((ext_vector_type(2)));
            __amdgpu_buffer_rsrc_t rsw = buf_rsrc(ws + (long)unit * Z * SLOT, Z * SLOT * 4);
            if (owner) {
#pragma unroll
                for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                    for (int g4 = 0; g4 < 4; ++g4) {
                        u32x4 val;
                        val.x = __float_as_uint(oacc[dt][4 * g4]); val.y = __float_as_uint(oacc[dt][4 * g4 + 1]);
                        val.z = __float_as_uint(oacc[dt][4 * g4 + 2]); val.w = __float_as_uint(oacc[dt][4 * g4 + 3]);
                        __builtin_amdgcn_raw_buffer_store_b128(val, rsw, (z * SLOT + (((grp * 2 + dt) * 4 + g4) * 64 + lane) * 4) * 4, 0, 16);
                    }
                u2 st2; st2.x = __float_as_uint(m_run); st2.y = __float_as_uint(l_run);
                __builtin_amdgcn_raw_buffer_store_b64(st2, rsw, (z * SLOT + 2 * 32 * 64 + (grp * 64 + lane) * 2) * 4, 0, 16);
            }
            wait_vm<0>();
            __syncthreads();
            int* ticket = reinterpret_cast<int*>(stats + 2 * 64 * 2);
            if (tid == 0) *ticket = __hip_atomic_fetch_add(cnt + unit, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            if (*ticket != Z - 1) return;                            // not the last slice of this query tile
            if (tid == 0) __hip_atomic_store(cnt + unit, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (!owner) return;
            float mz[4], lz[4], M = -INFINITY;
#pragma unroll
            for (int zz = 0; zz < 4; ++zz) {
                mz[zz] = -INFINITY; lz[zz] = 0.f;
                if (zz < Z) {
                    if (zz == z) { mz[zz] = m_run; lz[zz] = l_run; }
                    else {
                        const u2 st2 = __builtin_amdgcn_raw_buffer_load_b64(rsw, (zz * SLOT + 2 * 32 * 64 + (grp * 64 + lane) * 2) * 4, 0, 16);
                        mz[zz] = __uint_as_float(st2.x); lz[zz] = __uint_as_float(st2.y);
                    }
                    M = fmaxf(M, mz[zz]);
                }
            }
            f32x16 osum[2];
#pragma unroll
            for (int r = 0; r < 16; ++r) { osum[0][r] = 0.f; osum[1][r] = 0.f; }
            float lsum = 0.f;
#pragma unroll
            for (int zz = 0; zz < 4; ++zz) {
                if (zz >= Z) break;
                const float sc = mz[zz] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mz[zz] - M);
                lsum += lz[zz] * sc;
                if (zz == z) {
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) osum[dt][r] += oacc[dt][r] * sc;
                } else {
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                        for (int g4 = 0; g4 < 4; ++g4) {
                            const u32x4 val = __builtin_amdgcn_raw_buffer_load_b128(rsw, (zz * SLOT + (((grp * 2 + dt) * 4 + g4) * 64 + lane) * 4) * 4, 0, 16);
                            osum[dt][4 * g4] += __uint_as_float(val.x) * sc; osum[dt][4 * g4 + 1] += __uint_as_float(val.y) * sc;
                            osum[dt][4 * g4 + 2] += __uint_as_float(val.z) * sc; osum[dt][4 * g4 + 3] += __uint_as_float(val.w) * sc;
                        }
                }
            }
            oacc[0] = osum[0]; oacc[1] = osum[1];
            l_run = lsum;
        }
    }
    if (!owner) return;
    // ---- normalise + store o[b][n][h*64 + d] ---------------------------------------------------------
    const int qr = q0 + lr;
    if (qr < N) {
        // VARLEN: rows >= NL leave as 0 x O (finite: zero for a dead tile, an average of live V rows otherwise) — a scale, not a
        // select in front of the conversion, so that the live rows keep the uniform kernel's instruction forms (f16: multiply,
        // then convert; a select in between made the compiler fuse them into one rounding elsewhere)
        const float inv = VARLEN && qr >= NL ? 0.f : 1.0f / l_run;
        const int b = bh / H, h = bh - b * H;
        T* ob = o + ((long)b * N + qr) * H * D + h * D;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                T vals[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) vals[e] = from_f32<T>(oacc[dt][g * 4 + e] * inv);
                T* dst = ob + dt * 32 + 8 * g + 4 * hi;
                if constexpr (sizeof(T) == 4) *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(vals);
                else *reinterpret_cast<uint2*>(dst) = *reinterpret_cast<const uint2*>(vals);
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// attn_x3f_kernel — fp32 attention with BOTH products as exact three-way bf16 splits (the arithmetic of gemm_x3.hip).
// Layout and tiling of the 16-bit kernel above (V arrives transposed, [bh][64][v_ld]; K planes [key][64 + 8], V planes
// [d][64 + 4] in LDS), with fp32 in HBM: K and V^T are split ONCE per 64-key stage on their way into LDS (three bf16 planes
// each, shared by the four waves — 22 VALU instructions per float4 instead of a split per wave and tile), Q once per
// workgroup, the probabilities per tile.  Per 32x32 tile: 24 + 24 v_mfma_f32_32x32x16_bf16 (1536 matrix-core cycles)
// against 32 + 32 v_mfma_f32_32x32x2_f32 (4096).  SPLIT2 / key slices / merge: as attn_kernel.
// ---------------------------------------------------------------------------------------------------------------------
// KVP: K and V^T arrive ALREADY split, as the three bf16 planes the QKV epilogue wrote (k = [bh][3][kld][64] bf16,
// v = [bh][3][64][vld] bf16, kld = vld = N rounded up to the 64-key stage): a stage is 12 16-byte loads per thread copied to
// LDS as they are, instead of 8 float4 loads + 176 VALU of splitting per thread and stage — work that every one of the
// N / 64 query tiles of a head repeated on the same K / V values (with the key-split 64-query workgroups a wave multiplies
// ONE 32x32 tile per stage: the stage split was as many VALU cycles as the tile's softmax and P split together).
// NP = 2 (only with KVP): K / V^T arrive as fp16 {hi, lo} pairs with the low part UNSCALED (x3_split.h: x2u_split_pair — the
// operands of attention are of order one, their residuals stay above fp16's subnormal floor where it matters) and Q / P are
// split the same way: three partial products per block, small terms first, into the one accumulator — half the MFMAs of the
// three-plane form, 4 instead of 6 bytes per K / V element, no second accumulator set.
// VROWS (only with KVP): V arrives as rows like K, v = [bh][NP][kld][64] — the QKV epilogue then has no transposing branch for
// V (its 2-byte stores, 32 different rows per instruction, were ~4 us of that launch).  A stage of V is copied to LDS exactly like
// K, one 16-byte store per unit, into plain 128-byte rows [key][64 d] whose 16-byte chunk index is XORed with 4 * ((key >> 1) & 1);
// the P V operand (d along the lanes, eight keys per lane) comes out of the transposing LDS read of gfx950, two reads per
// fragment as before.  Bank arithmetic (bank = (byte / 4) mod 64 over a 32-lane half, 4 keys x 32 d per half): key parity selects
// the 128-byte half of the bank row, the XOR moves keys 2, 3 of a block onto the other 64 bytes, the 32 d are 64 contiguous bytes:
// every bank once.  The 16-byte stage stores cover one whole row per eight lanes whatever the XOR: conflict-free too.  The
// fragment holds the same keys in the same element order as the V^T form (keys 16 s2 + 4 hi + {0..3} and + 8), so the MFMA sequence
// and every operand are unchanged: results are bit-identical to the V^T layout.  Rows of the global planes past N may hold any
// bytes (another mode's, another length's): the last stage clears whole units by their key row, not by what the buffer holds.
typedef unsigned attn_u2 __attribute__((ext_vector_type(2)));
// one transposing read: per 16-lane group a block of 4 rows x 16 columns of 16-bit elements; lane 4q + p of the group supplies the
// (8-byte aligned) address of row q, columns 4p .. 4p + 3, lane i receives column i, row q in element q.  EXEC must be all ones.
// Inline asm: the compiler does NOT wait for it (attn_tr_wait).
template <int OFF> __device__ __forceinline__ void attn_lds_rd64_tr16(attn_u2& d, unsigned a) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(d) : "v"(a), "n"(OFF) : "memory");
#endif
}
__device__ __forceinline__ void attn_tr_wait() {
#if defined(__HIP_DEVICE_COMPILE__)
    wait_lgkm<0>();
#endif
}
// after attn_tr_wait(): volatile asm statements keep their order, so a use of d cannot move above the wait.  This rests on the
// compiler placing no copy or spill of d between the read and the wait (it cannot know that d is still in flight there): the VROWS
// instantiations build without spills (tools/kernel_resources.py) — check that again after any change that adds register pressure.
__device__ __forceinline__ void attn_tr_use(attn_u2& d) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(d));
#endif
}
template <int N, int I = 0, typename F> __device__ __forceinline__ void attn_unroll(F&& f) {
    if constexpr (I < N) { f(std::integral_constant<int, I>{}); attn_unroll<N, I + 1>(f); }
}
// the 2 x NP fragments of the keys 16 S2 .. 16 S2 + 15 of a 32-key tile: a0 / a1 = the lane's address for head-dim half 0 / 1 in
// plane 0 at the tile's first key; PLB = bytes per plane.  Low planes first: the order in which the products use them.
template <int NP, int PLB, int S2> __device__ __forceinline__ void attn_v_tr_read(attn_u2 (&t)[2][NP][2], unsigned a0, unsigned a1) {
    attn_unroll<NP>([&](auto PL) {
        constexpr int pl = NP - 1 - decltype(PL)::value, o = pl * PLB + S2 * 16 * 128;
        attn_lds_rd64_tr16<o>(t[0][pl][0], a0); attn_lds_rd64_tr16<o + 8 * 128>(t[0][pl][1], a0);
        attn_lds_rd64_tr16<o>(t[1][pl][0], a1); attn_lds_rd64_tr16<o + 8 * 128>(t[1][pl][1], a1);
    });
}
#if defined(MI355TTS_ATTN_TRACE)      // tuning only: s_memtime stamps at the phase boundaries of one wave (tools/dbg/attn_trace.sh)
#define TSTAMP(v) do { __builtin_amdgcn_sched_barrier(0); asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) :: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)
#define TACC(k, t1, t0) tr_[k] += (t1) - (t0)
#else
#define TSTAMP(v) do { } while (0)
#define TACC(k, t1, t0) do { } while (0)
#endif
template <bool SPLIT2, bool KVP = false, int NP = 3, bool VARLEN = false, bool VROWS = false>
__global__ __launch_bounds__(256, NP == 2 ? 3 : 2) void attn_x3f_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                       const float* __restrict__ v, float* __restrict__ o, int H, int N,
                                                       float* __restrict__ ws, int* __restrict__ cnt,
                                                       unsigned char* __restrict__ o_planes, int o_np, int xmap = 0,
                                                       int cut1 = 0, int cut2 = 0, int cut3 = 0, const int* __restrict__ lens = nullptr) {
    ATTN_XCD_MAP
    // o_planes != null: the output leaves as gemm_x3p.hip panel planes of the [B * N][H * 64] matrix (the A operand of the O
    // projection), split here (o_np = 3 bf16 planes | 2 fp16 planes), instead of fp32 rows in o
    static_assert(NP == 3 || (NP == 2 && KVP), "attn_x3f: the two-plane form reads pre-split K / V");
    static_assert(!VROWS || KVP, "attn_x3f: V as rows is a layout of the pre-split planes");
    using MF = std::conditional_t<NP == 3, Mfma<bf16>, Mfma<f16>>;
    using Frag = typename MF::Frag;
    constexpr int D = 64, KT = 64;
    constexpr int LDK = D + 8, LDV = VROWS ? D : KT + 4;    // bf16 elements per plane row (VROWS: V rows are keys, unpadded, chunks XORed)
    constexpr int KPL = KT * LDK, VPL = VROWS ? KT * LDV : D * LDV;            // elements per plane
    static_assert((NP * KPL * 2) % 16 == 0 && (VPL * 2) % 16 == 0, "attn_x3f: 16-byte aligned V planes");
    __shared__ __attribute__((aligned(16))) bf16 smem[NP * KPL + NP * VPL];            // 16-bit storage (bf16 or fp16 bit patterns)
    static_assert(sizeof(smem) >= (2 * 32 * 64 + 2 * 64 * 2 + 4) * sizeof(float), "merge buffer fits the stage");
    bf16* Ks = smem;
    bf16* Vs = smem + NP * KPL;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 31, hi = lane >> 5;
    const int bh = by_;
    ATTN_VARLEN_PROLOGUE
    const int q0 = SPLIT2 ? bx_ * 64 + (wave >> 1) * 32 : bx_ * 128 + wave * 32;
    const float* qb = q + (long)bh * N * D;
    const float* kb = k + (long)bh * N * D;
    const long vld = KVP ? (long)((N + 63) / 64 * 64) : (long)((N + 7) / 8 * 8);
    const float* vb = v + (long)bh * D * vld;
    const bf16* kpb = reinterpret_cast<const bf16*>(k) + (long)bh * NP * vld * D;     // KVP: planes [NP][kld][64], kld = vld
    const bf16* vpb = reinterpret_cast<const bf16*>(v) + (long)bh * NP * D * vld;     // KVP: planes [NP][64][vld]

    auto split4 = [&](const float4 a, uint2& w1, uint2& w2, uint2& w3) __attribute__((always_inline)) {
        x3_split_pair(a.x, a.y, w1.x, w2.x, w3.x);
        x3_split_pair(a.z, a.w, w1.y, w2.y, w3.y);
    };
    auto split8 = [&](const float4 a, const float4 b, Frag& f1, Frag& f2, Frag& f3) __attribute__((always_inline)) {
        uint2 a1, a2, a3, b1, b2, b3;
        split4(a, a1, a2, a3); split4(b, b1, b2, b3);
        f1 = __builtin_bit_cast(Frag, u32x4{a1.x, a1.y, b1.x, b1.y});
        f2 = __builtin_bit_cast(Frag, u32x4{a2.x, a2.y, b2.x, b2.y});
        f3 = __builtin_bit_cast(Frag, u32x4{a3.x, a3.y, b3.x, b3.y});
    };

    auto split8h = [&](const float4 a, const float4 b, Frag& f1, Frag& f2) __attribute__((always_inline)) {
        unsigned h[4], l[4];
        x2u_split_pair(a.x, a.y, h[0], l[0]); x2u_split_pair(a.z, a.w, h[1], l[1]);
        x2u_split_pair(b.x, b.y, h[2], l[2]); x2u_split_pair(b.z, b.w, h[3], l[3]);
        f1 = __builtin_bit_cast(Frag, u32x4{h[0], h[1], h[2], h[3]});
        f2 = __builtin_bit_cast(Frag, u32x4{l[0], l[1], l[2], l[3]});
    };
    // the probabilities: in [0, 1] by construction, no range clamp
    auto split8p = [&](const float4 a, const float4 b, Frag& f1, Frag& f2) __attribute__((always_inline)) {
        unsigned h[4], l[4];
        x2u_split_pair_raw_mix(a.x, a.y, h[0], l[0]); x2u_split_pair_raw_mix(a.z, a.w, h[1], l[1]);
        x2u_split_pair_raw_mix(b.x, b.y, h[2], l[2]); x2u_split_pair_raw_mix(b.z, b.w, h[3], l[3]);
        f1 = __builtin_bit_cast(Frag, u32x4{h[0], h[1], h[2], h[3]});
        f2 = __builtin_bit_cast(Frag, u32x4{l[0], l[1], l[2], l[3]});
    };

    // ---- Q: the NP pieces of log2(e) * Q[q0 + lr][16 ks + 8 hi .. +8] ------------------------------------------------
    Frag qf3[4][NP];
    {
        const int qr = q0 + lr;
        const bool ok = qr < NL;
        constexpr float L2E = 1.4426950408889634f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            float4 a = float4{0.f, 0.f, 0.f, 0.f}, b = a;
            if (ok) {
                a = *reinterpret_cast<const float4*>(qb + (long)qr * D + ks * 16 + hi * 8);
                b = *reinterpret_cast<const float4*>(qb + (long)qr * D + ks * 16 + hi * 8 + 4);
            }
            a.x *= L2E; a.y *= L2E; a.z *= L2E; a.w *= L2E; b.x *= L2E; b.y *= L2E; b.z *= L2E; b.w *= L2E;
            if constexpr (NP == 3) split8(a, b, qf3[ks][0], qf3[ks][1], qf3[ks][2]); else split8h(a, b, qf3[ks][0], qf3[ks][1]);
        }
    }

    // ---- stage loads: 64 keys x 64 d of K (rows = keys) and of V (VROWS: rows = keys like K; else V^T, rows = d) ----------------
    float4 kreg[KVP ? 1 : 4], vreg[KVP ? 1 : 4];
    constexpr int NU = 2 * NP;                              // KVP: 16-byte units per thread and operand per stage
    u32x4 kpl[KVP ? NU : 1], vpl[KVP ? NU : 1];
    auto load_regs = [&](int key0) {
        if constexpr (KVP) {
            // unit u = tid + 256 i: plane u / 512 ; K (and V with VROWS): key (u % 512) / 8, 8 d's ; V^T: d (u % 512) / 8, 8 keys.
            // Keys past N are inside the padded planes and may hold any bytes, finite or not (another length's, another layout's):
            // K's scores are masked in the tile, V's values are cleared below
#pragma unroll
            for (int i = 0; i < NU; ++i) {
                const int u = tid + i * 256, pl = u >> 9, r = (u & 511) >> 3, c = u & 7;
                kpl[i] = *reinterpret_cast<const u32x4*>(kpb + ((long)pl * vld + key0 + r) * D + c * 8);
                if constexpr (VROWS) vpl[i] = *reinterpret_cast<const u32x4*>(vpb + ((long)pl * vld + key0 + r) * D + c * 8);
                else vpl[i] = *reinterpret_cast<const u32x4*>(vpb + ((long)pl * D + r) * vld + key0 + c * 8);
            }
            if (VROWS && key0 + KT > NL) {
                // last stage, V as rows: a unit is eight d's of ONE key — cleared whole when that key is >= NL (0 x NaN is NaN, and
                // the rows past N hold whatever the buffer held before)
#pragma unroll
                for (int i = 0; i < NU; ++i)
                    if (key0 + (((tid + i * 256) & 511) >> 3) >= NL) vpl[i] = u32x4{0u, 0u, 0u, 0u};
            } else if (key0 + KT > NL) {
                // last stage: the V^T values of keys >= N meet probabilities that are exactly zero, but 0 x NaN is NaN and
                // the pad columns hold whatever the buffer held before (another layout, another mode): clear them here
#pragma unroll
                for (int i = 0; i < NU; ++i) {
                    const int keep = NL - (key0 + ((tid + i * 256) & 7) * 8);         // valid keys among this unit's eight
                    if (keep < 8) {
                        unsigned w[4] = {vpl[i].x, vpl[i].y, vpl[i].z, vpl[i].w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) w[e] &= (2 * e < keep ? 0x0000ffffu : 0u) | (2 * e + 1 < keep ? 0xffff0000u : 0u);
                        vpl[i] = u32x4{w[0], w[1], w[2], w[3]};
                    }
                }
            }
        } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int vi = tid + i * 256;
            const int key = vi >> 4, dv = vi & 15;              // K: row key, floats 4 dv .. 4 dv + 3
            const int d = vi >> 4, kv = vi & 15;                // V^T: row d, keys key0 + 4 kv .. + 3
            float4 a = float4{0.f, 0.f, 0.f, 0.f}, b = a;
            if (key0 + key < NL) a = *reinterpret_cast<const float4*>(kb + (long)(key0 + key) * D + dv * 4);
            if (key0 + kv * 4 < NL) b = *reinterpret_cast<const float4*>(vb + (long)d * vld + key0 + kv * 4);
            if constexpr (VARLEN) {           // keys [NL, N) are padding rows of the slab: clear their V^T values
                const int keep = NL - (key0 + kv * 4);
                if (keep < 2) b.y = 0.f;
                if (keep < 3) b.z = 0.f;
                if (keep < 4) b.w = 0.f;
            }
            kreg[i] = a; vreg[i] = b;
        }
        }
    };
    auto store_lds = [&]() {
        if constexpr (KVP) {
#pragma unroll
            for (int i = 0; i < NU; ++i) {
                const int u = tid + i * 256, pl = u >> 9, r = (u & 511) >> 3, c = u & 7;
                *reinterpret_cast<u32x4*>(Ks + pl * KPL + r * LDK + c * 8) = kpl[i];                 // 144-byte rows: 16-byte aligned
                if constexpr (VROWS) {
                    *reinterpret_cast<u32x4*>(Vs + pl * VPL + r * LDV + ((c ^ ((r & 2) << 1)) * 8)) = vpl[i];   // 128-byte rows, chunk ^ 4 * ((key >> 1) & 1)
                } else {
                uint2* vd = reinterpret_cast<uint2*>(Vs + pl * VPL + r * LDV + c * 8);                // 136-byte rows: 8-byte aligned
                vd[0] = uint2{vpl[i].x, vpl[i].y}; vd[1] = uint2{vpl[i].z, vpl[i].w};
                }
            }
        } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int vi = tid + i * 256;
            const int r = vi >> 4, c = vi & 15;
            uint2 w1, w2, w3;
            split4(kreg[i], w1, w2, w3);
            *reinterpret_cast<uint2*>(Ks + r * LDK + c * 4) = w1;
            *reinterpret_cast<uint2*>(Ks + KPL + r * LDK + c * 4) = w2;
            *reinterpret_cast<uint2*>(Ks + 2 * KPL + r * LDK + c * 4) = w3;
            split4(vreg[i], w1, w2, w3);
            *reinterpret_cast<uint2*>(Vs + r * LDV + c * 4) = w1;
            *reinterpret_cast<uint2*>(Vs + VPL + r * LDV + c * 4) = w2;
            *reinterpret_cast<uint2*>(Vs + 2 * VPL + r * LDV + c * 4) = w3;
        }
        }
    };

    // VROWS: this lane's address in the transposed reads of V, plane 0, key 0 of the stage, head-dim half 0 / 1: block row q =
    // (lane >> 2) & 3 of keys 4 hi + q, columns 16 * ((lane >> 4) & 1) + 4 * (lane & 3) .. + 3 of the half (dt ^ (q >> 1): the XOR)
    unsigned vtr[2] = {0u, 0u};
    if constexpr (VROWS) {
        const int q4 = (lane >> 2) & 3;
        const unsigned a = lds_addr(Vs) + (4 * hi + q4) * (LDV * 2) + ((lane >> 4) & 1) * 32 + (lane & 3) * 8;
        vtr[0] = a + (q4 >> 1) * 64;
        vtr[1] = a + ((q4 >> 1) ^ 1) * 64;
    }
    f32x16 oacc[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { oacc[0][r] = 0.f; oacc[1][r] = 0.f; }
    float m_run = -INFINITY, l_run = 0.f;
#if defined(MI355TTS_ATTN_TRACE)
    unsigned long long tr_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ta_ = 0, tb_ = 0, tc_ = 0, td_ = 0, te_ = 0, tk_ = 0;
    TSTAMP(tk_);
#endif

    const int nstage_all = dead ? 0 : (NL + KT - 1) / KT;
    // key slices (gridDim.z > 1): see the merge below.  cut1 > 0 (round 6): UNEVEN slices [0, cut1), [cut1, cut2), ... chosen by the
    // launcher so that the z-major dispatch order is longest-piece-first on the 3 x CUs slots (attn_pick_slices)
    int st0 = (int)((long)blockIdx.z * nstage_all / gridDim.z);
    int nstage = (int)((long)(blockIdx.z + 1) * nstage_all / gridDim.z);
    if (cut1 > 0) {
        const int zz = (int)blockIdx.z, ZZ = (int)gridDim.z;
        st0 = zz == 0 ? 0 : zz == 1 ? cut1 : zz == 2 ? cut2 : cut3;
        nstage = zz + 1 == ZZ ? nstage_all : zz == 0 ? cut1 : zz == 1 ? cut2 : cut3;
    }
    if constexpr (VARLEN) { st0 = min(st0, nstage_all); nstage = min(nstage, nstage_all); }      // cuts are chosen for N stages
    if (st0 < nstage) {
        load_regs(st0 * KT);
        store_lds();
        __syncthreads();
    }
    constexpr int TA[6] = {0, 1, 2, 0, 1, 0}, TB[6] = {2, 1, 0, 1, 0, 0};      // piece pairs, small terms first
    for (int st = st0; st < nstage; ++st) {
        if (st + 1 < nstage) load_regs((st + 1) * KT);
        auto tile = [&](int kt) {
            const int key0 = st * KT + kt * 32;
            TSTAMP(ta_);
            // ---- S^T tile: 32 keys x 32 queries, six partial products per k16 step ---------------------------------------
            f32x16 sacc;
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                Frag kf[NP];
#pragma unroll
                for (int pl = 0; pl < NP; ++pl)
                    kf[pl] = *reinterpret_cast<const Frag*>(Ks + pl * KPL + (kt * 32 + lr) * LDK + ks * 16 + hi * 8);
                if constexpr (NP == 3) {
#pragma unroll
                    for (int t = 0; t < 6; ++t) sacc = MF::mma(kf[TA[t]], qf3[ks][TB[t]], sacc);
                } else {                          // small terms first, one accumulator (unscaled low parts)
                    sacc = MF::mma(kf[1], qf3[ks][0], sacc);
                    sacc = MF::mma(kf[0], qf3[ks][1], sacc);
                    sacc = MF::mma(kf[0], qf3[ks][0], sacc);
                }
            }
            if (key0 + 32 > NL) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = key0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    if (key >= NL) sacc[r] = -INFINITY;
                }
            }
            float mloc = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) mloc = fmaxf(mloc, sacc[r]);
            mloc = xor32_max(mloc);
#if defined(MI355TTS_ATTN_TRACE)
            { const float keep_ = mloc; asm volatile("" :: "v"(keep_)); }
#endif
            TSTAMP(tb_); TACC(0, tb_, ta_);            // K fragment reads + score MFMAs + tile maximum
            float alpha = 1.f;
            if (!__all(mloc - m_run <= 8.0f)) {
                const float m_new = fmaxf(m_run, mloc);
                alpha = __builtin_amdgcn_exp2f(m_run - m_new);
                m_run = m_new;
#pragma unroll
                for (int r = 0; r < 16; ++r) { oacc[0][r] *= alpha; oacc[1][r] *= alpha; }
            }
            // s - m and the row sum as SCALAR fp32 VALU: packed fp32 instructions beside MFMAs cost more than the two scalar ones they
            // replace (the float2 form of this loop, and the compiler's own pairing of adjacent scalar operations, measured
            // +0.66 ms per step: LOG.md round 7).  The empty asm statements keep the vectoriser from pairing them again.  Two
            // partial sums, even and odd registers, added at the end: the values and the order of the float2 form, bit-identical.
            float p[16];
            float ls0 = 0.f, ls1 = 0.f;
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                float d0 = sacc[r] - m_run, d1 = sacc[r + 1] - m_run;
                asm("" : "+v"(d0)); asm("" : "+v"(d1));
                p[r] = __builtin_amdgcn_exp2f(d0); p[r + 1] = __builtin_amdgcn_exp2f(d1);
                ls0 += p[r]; ls1 += p[r + 1];
                asm("" : "+v"(ls0)); asm("" : "+v"(ls1));
            }
            float lsum = ls0 + ls1;
            lsum = xor32_sum(lsum);
            l_run = l_run * alpha + lsum;
#if defined(MI355TTS_ATTN_TRACE)
            { const float keep_ = l_run + p[0] + p[15]; asm volatile("" :: "v"(keep_)); }
#endif
            TSTAMP(tc_); TACC(1, tc_, tb_);            // exponentials + row sum
            // ---- O^T += V^T P^T: the probabilities a lane holds are the B operand (keys in accumulator-row order) ------------
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                Frag pf[NP];
                if constexpr (NP == 3)
                    split8(float4{p[8 * s2], p[8 * s2 + 1], p[8 * s2 + 2], p[8 * s2 + 3]},
                           float4{p[8 * s2 + 4], p[8 * s2 + 5], p[8 * s2 + 6], p[8 * s2 + 7]}, pf[0], pf[1], pf[2]);
                else
                    split8p(float4{p[8 * s2], p[8 * s2 + 1], p[8 * s2 + 2], p[8 * s2 + 3]},
                            float4{p[8 * s2 + 4], p[8 * s2 + 5], p[8 * s2 + 6], p[8 * s2 + 7]}, pf[0], pf[1]);
                // the two head-dim halves alternate: an MFMA that waits for the previous one's accumulator costs 52 cycles instead
                // of 32 (tools/ubench/mfma_valu_coexec.hip); the order inside each accumulator is unchanged (bit-identical).
                // (The same for the two score tiles of a stage in the 128-query form was measured too: 27 spilled registers and
                // the stage loads issued one tile later cost more than the chains gain, 56.9 -> 70.8 us.)
                Frag vf[2][NP];
                if constexpr (VROWS) {
                    // the same eight keys per lane, in the same order, as the two 8-byte row reads of the V^T image below
                    attn_u2 t[2][NP][2];
                    const unsigned a0 = vtr[0] + kt * (32 * LDV * 2), a1 = vtr[1] + kt * (32 * LDV * 2);
                    if (s2 == 0) attn_v_tr_read<NP, VPL * 2, 0>(t, a0, a1); else attn_v_tr_read<NP, VPL * 2, 1>(t, a0, a1);
                    attn_tr_wait();
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                        for (int pl = 0; pl < NP; ++pl) {
                            attn_tr_use(t[dt][pl][0]); attn_tr_use(t[dt][pl][1]);
                            vf[dt][pl] = __builtin_bit_cast(Frag, u32x4{t[dt][pl][0].x, t[dt][pl][0].y, t[dt][pl][1].x, t[dt][pl][1].y});
                        }
                } else {
#pragma unroll
                for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                    for (int pl = 0; pl < NP; ++pl) {
                        const bf16* row = Vs + pl * VPL + (dt * 32 + lr) * LDV + kt * 32 + 16 * s2 + 4 * hi;
                        uint2 a2[2];
                        a2[0] = *reinterpret_cast<const uint2*>(row);
                        a2[1] = *reinterpret_cast<const uint2*>(row + 8);
                        vf[dt][pl] = __builtin_bit_cast(Frag, u32x4{a2[0].x, a2[0].y, a2[1].x, a2[1].y});
                    }
                }
                if constexpr (NP == 3) {
#pragma unroll
                    for (int t = 0; t < 6; ++t)
#pragma unroll
                        for (int dt = 0; dt < 2; ++dt) oacc[dt] = MF::mma(vf[dt][TA[t]], pf[TB[t]], oacc[dt]);
                } else {
                    oacc[0] = MF::mma(vf[0][1], pf[0], oacc[0]);
                    oacc[1] = MF::mma(vf[1][1], pf[0], oacc[1]);
                    oacc[0] = MF::mma(vf[0][0], pf[1], oacc[0]);
                    oacc[1] = MF::mma(vf[1][0], pf[1], oacc[1]);
                    oacc[0] = MF::mma(vf[0][0], pf[0], oacc[0]);
                    oacc[1] = MF::mma(vf[1][0], pf[0], oacc[1]);
                }
            }
            TSTAMP(td_); TACC(2, td_, tc_);            // P split + V fragment reads + P V MFMAs (issued)
        };
        if constexpr (SPLIT2) {
            if (st * KT + (wave & 1) * 32 < NL) tile(wave & 1);
        } else {
#pragma unroll
            for (int kt = 0; kt < KT / 32; ++kt) {
                const int key0 = st * KT + kt * 32;
                if (key0 < NL) tile(kt);
            }
        }
        TSTAMP(ta_);
        __syncthreads();
        TSTAMP(tb_); TACC(3, tb_, ta_);                // barrier 1 (includes the tail of the P V MFMAs)
        if (st + 1 < nstage) {
            store_lds();
            TSTAMP(tc_); TACC(4, tc_, tb_);            // wait for the stage loads + LDS stores
            __syncthreads();
            TSTAMP(te_); TACC(5, te_, tc_);            // barrier 2
        }
    }
#if defined(MI355TTS_ATTN_TRACE)
    TSTAMP(te_);
    if (blockIdx.x == 3 && blockIdx.y == 5 && (threadIdx.x & 63) == 0)
        printf("ATTN_TRACE z %d wave %d stages %d total %llu | S+max %llu exp %llu PV %llu bar1 %llu store %llu bar2 %llu\n", (int)blockIdx.z, wave, nstage - st0,
               te_ - tk_, tr_[0], tr_[1], tr_[2], tr_[3], tr_[4], tr_[5]);
#endif
    bool owner = true;                                              // this wave holds a finished 32-query result
    constexpr int NG = SPLIT2 ? 2 : 4;                              // 32-query groups of the workgroup
    int grp = wave;
    float* comb = reinterpret_cast<float*>(smem);                   // [2 groups][32 accumulator registers][64 lanes] (SPLIT2 pair merge)
    float* stats = comb + 2 * 32 * 64;                              // [2 groups][64 lanes][m, l]
    if constexpr (SPLIT2) {
        // ---- merge the two key halves: m = max(m0, m1) ; l = l0 2^(m0-m) + l1 2^(m1-m) ; O likewise ----------------------
        __syncthreads();                                            // every wave is done with the K / V stage
        grp = wave >> 1;
        owner = !(wave & 1);
        if (!owner) {
            stats[(grp * 64 + lane) * 2] = m_run; stats[(grp * 64 + lane) * 2 + 1] = l_run;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) comb[((grp * 2 + dt) * 16 + r) * 64 + lane] = oacc[dt][r];
        }
        __syncthreads();
        if (owner) {
            const float m1 = stats[(grp * 64 + lane) * 2], l1 = stats[(grp * 64 + lane) * 2 + 1];
            const float m = fmaxf(m_run, m1);
            const float s0 = m_run == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m_run - m);
            const float s1 = m1 == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m1 - m);
            l_run = l_run * s0 + l1 * s1;
            m_run = m;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[dt][r] = oacc[dt][r] * s0 + comb[((grp * 2 + dt) * 16 + r) * 64 + lane] * s1;
        }
    }
    {
        // ---- key slices (gridDim.z > 1).  One utterance in fp32 is 18 x 32 = 576 of these workgroups on 768 slots (three per
        // CU): 2.25 per CU, so the CUs that got three set the makespan and a quarter of the chip idles.  With Z slices the
        // work comes in pieces of 1 / Z (Z = 4: exactly 9 per CU).  Every slice publishes (m, l, O) of its keys with
        // write-through stores, drains them, and takes a ticket (relaxed agent-scope fetch-add: the gemm_sk.hip hand-off);
        // the workgroup that draws the last ticket adds the slices IN SLICE ORDER (its own from registers), so the result
        // does not depend on which one that is, resets the ticket counter (hipGraph replays find it at zero) and stores.
        // Nobody waits for anybody: there is no residency requirement. ---------------------------------------------------
        const int Z = (int)gridDim.z;
        if (Z > 1 && !dead) {                                        // (a tile with no live query takes no ticket: see ATTN_VARLEN_PROLOGUE)
            const int z = (int)blockIdx.z;
            const int unit = (int)(by_ * gridDim.x + bx_);
            constexpr int SLOT = NG * (32 * 64 + 64 * 2);            // floats per (unit, slice)
            // write-through (sc1) stores / sc1 loads through a buffer descriptor, as in gemm_sk.hip: no L2-wide write-back fence
            typedef unsigned int u2 __attribute__((ext_vector_type(2)));
            __amdgpu_buffer_rsrc_t rsw = buf_rsrc(ws + (long)unit * Z * SLOT, Z * SLOT * 4);
            if (owner) {
#pragma unroll
                for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                    for (int g4 = 0; g4 < 4; ++g4) {
                        u32x4 val;
                        val.x = __float_as_uint(oacc[dt][4 * g4]); val.y = __float_as_uint(oacc[dt][4 * g4 + 1]);
                        val.z = __float_as_uint(oacc[dt][4 * g4 + 2]); val.w = __float_as_uint(oacc[dt][4 * g4 + 3]);
                        __builtin_amdgcn_raw_buffer_store_b128(val, rsw, (z * SLOT + (((grp * 2 + dt) * 4 + g4) * 64 + lane) * 4) * 4, 0, 16);
                    }
                u2 st2; st2.x = __float_as_uint(m_run); st2.y = __float_as_uint(l_run);
                __builtin_amdgcn_raw_buffer_store_b64(st2, rsw, (z * SLOT + NG * 32 * 64 + (grp * 64 + lane) * 2) * 4, 0, 16);
            }
            wait_vm<0>();
            __syncthreads();                                         // (also: every wave is done with the K / V stage the ticket word lies in)
            int* ticket = reinterpret_cast<int*>(stats + 2 * 64 * 2);
            if (tid == 0) *ticket = __hip_atomic_fetch_add(cnt + unit, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            if (*ticket != Z - 1) return;                            // not the last slice of this query tile
            if (tid == 0) __hip_atomic_store(cnt + unit, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (!owner) return;
            float mz[4], lz[4], M = -INFINITY;
#pragma unroll
            for (int zz = 0; zz < 4; ++zz) {
                mz[zz] = -INFINITY; lz[zz] = 0.f;
                if (zz < Z) {
                    if (zz == z) { mz[zz] = m_run; lz[zz] = l_run; }
                    else {
                        const u2 st2 = __builtin_amdgcn_raw_buffer_load_b64(rsw, (zz * SLOT + NG * 32 * 64 + (grp * 64 + lane) * 2) * 4, 0, 16);
                        mz[zz] = __uint_as_float(st2.x); lz[zz] = __uint_as_float(st2.y);
                    }
                    M = fmaxf(M, mz[zz]);
                }
            }
            f32x16 osum[2];
#pragma unroll
            for (int r = 0; r < 16; ++r) { osum[0][r] = 0.f; osum[1][r] = 0.f; }
            float lsum = 0.f;
#pragma unroll
            for (int zz = 0; zz < 4; ++zz) {
                if (zz >= Z) break;
                const float sc = mz[zz] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mz[zz] - M);
                lsum += lz[zz] * sc;
                if (zz == z) {
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) osum[dt][r] += oacc[dt][r] * sc;
                } else {
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                        for (int g4 = 0; g4 < 4; ++g4) {
                            const u32x4 val = __builtin_amdgcn_raw_buffer_load_b128(rsw, (zz * SLOT + (((grp * 2 + dt) * 4 + g4) * 64 + lane) * 4) * 4, 0, 16);
                            osum[dt][4 * g4] += __uint_as_float(val.x) * sc; osum[dt][4 * g4 + 1] += __uint_as_float(val.y) * sc;
                            osum[dt][4 * g4 + 2] += __uint_as_float(val.z) * sc; osum[dt][4 * g4 + 3] += __uint_as_float(val.w) * sc;
                        }
                }
            }
            oacc[0] = osum[0]; oacc[1] = osum[1];
            l_run = lsum;
        }
    }
    if (!owner) return;
    // ---- normalise + store o[b][n][h*64 + d] ---------------------------------------------------------
    const int qr = q0 + lr;
    if (qr < N) {
        const float inv = VARLEN && qr >= NL ? 0.f : 1.0f / l_run;          // VARLEN: rows >= NL leave as zeros (see attn_kernel)
        const int b = bh / H, h = bh - b * H;
        float* ob = o + ((long)b * N + qr) * H * D + h * D;
        const long row = (long)b * N + qr;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float vals[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) vals[e] = (oacc[dt][g * 4 + e] * inv);
                if (o_planes) {
                    // columns h*64 + dt*32 + 8g + 4hi .. +3: half (8 bytes) of the k-slot s8 = h*8 + dt*4 + g of every plane
                    uint2 w1, w2, w3;
                    unsigned char* dst = o_planes + x3p_slot_offset(row, h * 8 + dt * 4 + g, (H * D) >> 5, o_np) + 8 * hi;
                    if (o_np == 3) {
                        x3_split_pair(vals[0], vals[1], w1.x, w2.x, w3.x);
                        x3_split_pair(vals[2], vals[3], w1.y, w2.y, w3.y);
                        *reinterpret_cast<uint2*>(dst + 2 * X3P_PLANE) = w3;
                    } else {
                        x2_split_pair(vals[0], vals[1], w1.x, w2.x);
                        x2_split_pair(vals[2], vals[3], w1.y, w2.y);
                    }
                    *reinterpret_cast<uint2*>(dst) = w1;
                    *reinterpret_cast<uint2*>(dst + X3P_PLANE) = w2;
                } else {
                    float* dst = ob + dt * 32 + 8 * g + 4 * hi;
                    *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(vals);
                }
            }
    }
}

// ---- host side: the plan, then the launch ------------------------------------------------------------------------------------
// attention_plan() reads the options and the engine's arithmetic (ArithScope, common.h) ONCE per evaluation, before the QKV
// projection, and its answer serves both sides: F5::dit_eval copies plan.kv into the QKV ConvGemm and hands the same plan to
// launch_attention(), which only launches.  (Five separate query functions used to be asked at different moments; a lazy option
// read inside the launcher once made the first block write V transposed for a kernel that then read it untransposed.)
// attn_f32_x3: 0 = native fp32 MFMA ; 1 = q.k as exact bf16 splits (attn_kernel X3S) ; 2 = both products (attn_x3f_kernel; V then
// arrives transposed like in the 16-bit engines)
static inline int opt_attn_x3() { const int o = arith_tls().attn_x3; return o >= 0 ? o : (int)opt(OPT_ATTN_F32_X3); }      // the engine's arithmetic first
static inline int opt_attn_np() { const int o = arith_tls().attn_np; return (o == 2 || o == 3) ? o : (int)opt(OPT_ATTN_F32_PLANES); }

AttnKvLayout attention_kv_layout(int N, int dtype, bool caller_can_presplit_kv) {
    AttnKvLayout l;
    const bool x3f = dtype == MI_F32 && opt_attn_x3() == 2;
    if (x3f && caller_can_presplit_kv && opt(OPT_ATTN_KV_PLANES) != 0) {
        l.kv_planes = opt_attn_np();
        l.k_ld = l.v_ld = (long)((N + ATTN_STAGE - 1) / ATTN_STAGE * ATTN_STAGE);
        l.v_rows = opt(OPT_ATTN_V_ROWS) != 0;
    } else if (x3f || dtype != MI_F32)
        l.v_ld = (long)((N + 7) / 8 * 8);
    return l;
}

// Key slices of the 128-query fp32 kernel, sized for the dispatch order (round 6).  The launch is (query tiles x heads) units x Z
// slices on 3 x CUs workgroup slots, dispatched z-major.  Equal slices make 288 x 3 = 864 workgroups for one utterance: a full
// round of 768 and an eighth of a second one, which costs as much as half a round (the second round's workgroups run alone on their
// SIMDs: ~18 of the launch's 50 us).  With slices of 7, 7 and 4 stages the long pieces start first and the short ones fill the slots
// they free: list scheduling, makespan 8 stage times instead of 12.  The search simulates that for every non-increasing split of the
// stages into 1 .. zmax slices (identical pieces handled in bulk: a few map operations per split) and keeps the best.
struct AttnSlices { int Z = 1, cut[3] = {0, 0, 0}; };
static AttnSlices attn_search_slices(long units, int S, int slots, int zmax) {
    AttnSlices best;
    double best_t = 1e30;
    auto makespan = [&](const int* len, int Z) -> double {
        std::map<double, long> free_at;                          // time -> slots that become free then
        free_at[0.0] = slots;
        double end = 0.0;
        for (int z = 0; z < Z; ++z) {
            const double cost = len[z] + (Z > 1 ? 0.6 : 0.3);      // stages + prologue / publish / merge (in stage times)
            long left = units;
            while (left > 0) {
                auto it = free_at.begin();
                const long take = std::min(left, it->second);
                const double t = it->first + cost;
                it->second -= take;
                if (it->second == 0) free_at.erase(it);
                free_at[t] += take;
                end = std::max(end, t);
                left -= take;
            }
        }
        return end;
    };
    int len[4];
    for (int Z = 1; Z <= zmax; ++Z) {
        if (S < 2 * Z && Z > 1) break;
        // non-increasing len[0] >= ... >= len[Z-1] >= 1 with sum S
        std::function<void(int, int, int)> rec = [&](int i, int left, int cap) {
            if (i == Z - 1) {
                if (left < 1 || left > cap) return;
                len[i] = left;
                const double t = makespan(len, Z);
                if (t < best_t - 1e-9) {
                    best_t = t; best.Z = Z;
                    int acc = 0;
                    for (int c = 0; c < 3; ++c) { acc += c < Z ? len[c] : 0; best.cut[c] = c + 1 < Z ? acc : S; }
                }
                return;
            }
            for (int a = std::min(cap, left - (Z - 1 - i)); a >= (left + (Z - i) - 1) / (Z - i); --a) { len[i] = a; rec(i + 1, left - a, a); }
        };
        rec(0, S, S);
    }
    return best;
}

// ... remembered per argument tuple: everything the result depends on is in the key
static AttnSlices attn_pick_slices(long units, int S, int slots, int zmax) {
    static std::mutex mu;
    static std::map<std::tuple<long, int, int, int>, AttnSlices> cache;
    std::lock_guard<std::mutex> lk(mu);
    const auto key = std::make_tuple(units, S, slots, zmax);
    auto it = cache.find(key);
    if (it == cache.end()) it = cache.emplace(key, attn_search_slices(units, S, slots, zmax)).first;
    return it->second;
}

// Even key slices: makespan(Z) = ceil(units * Z / CUs) / Z in units of one unsliced workgroup, + 6 % per extra slice for the
// prologue and the merge (measured, fp32, one utterance = 576 units: Z = 1 / 2 / 3 / 4 -> 135 / 122 / 121 / 126 us in round 2;
// 62.1 / 58.8 / 60.8 / 60.7 us with the fp16-pair kernel of round 3, whose slices are shorter against the same merge: + 9 % for fp32).
// A slice count must fit the workspace: units x Z slots of `slot` floats and one counter per unit.
static int attn_pick_z(long units, long slot, int nstage, bool f32, int zmax, long ws_floats, long cnt_n) {
    auto fits = [&](int z) { return units * z * slot <= ws_floats && units <= cnt_n; };
    if (const int zf = opt(OPT_ATTN_Z_FORCE); zf > 0) return fits(zf) ? zf : 1;
    const int cus = device_cus();
    int Z = 1;
    double best = 1e30;
    for (int z = 1; z <= zmax; ++z) {
        if (z > 1 && (!fits(z) || nstage < 2 * z)) break;
        const double cost = (double)((units * z + cus - 1) / cus) / z * (1.0 + (f32 ? 0.09 : 0.06) * (z - 1));
        if (cost < best - 1e-9) { best = cost; Z = z; }
    }
    return Z;
}

// ---- the dispatch table: one entry per AttnForm (+ SPLIT2), {profiler label, launch thunk [lengths][V as rows]} ---------------------
// lengths: the VARLEN instantiation (ragged batch, ATTN_VARLEN_PROLOGUE).  V as rows (AttnKvLayout::v_rows) exists for the pre-split
// forms only: the other entries have no thunk there.
struct AttnArgs { const AttnPlan& p; const void *q, *k, *v; void *o, *o_planes; int o_np; float* ws; int* cnt; const int* lens; hipStream_t s; };
using AttnThunk = void (*)(const AttnArgs&);
static dim3 attn_grid(const AttnPlan& p) { return dim3(p.grid[0], p.grid[1], p.grid[2]); }
template <typename T, bool SPLIT2, bool X3S, bool REFH, bool VARLEN> static void attn_go(const AttnArgs& a) {
    hipLaunchKernelGGL((attn_kernel<T, SPLIT2, X3S, REFH, VARLEN>), attn_grid(a.p), dim3(256), 0, a.s, (const T*)a.q, (const T*)a.k, (const T*)a.v,
                       (T*)a.o, a.p.H, a.p.N, a.ws, a.cnt, a.p.sscale, a.p.xmap, a.lens);
}
template <bool SPLIT2, bool KVP, int NP, bool VARLEN, bool VROWS> static void x3f_go(const AttnArgs& a) {
    hipLaunchKernelGGL((attn_x3f_kernel<SPLIT2, KVP, NP, VARLEN, VROWS>), attn_grid(a.p), dim3(256), 0, a.s, (const float*)a.q, (const float*)a.k,
                       (const float*)a.v, (float*)a.o, a.p.H, a.p.N, a.ws, a.cnt, (unsigned char*)a.o_planes, a.o_np, a.p.xmap, a.p.cut[0], a.p.cut[1],
                       a.p.cut[2], a.lens);
}
struct AttnEntry { const char* label; AttnThunk go[2][2]; };
#define ATTN_ROWS(T, SP, X3S, REFH) {{attn_go<T, SP, X3S, REFH, false>, nullptr}, {attn_go<T, SP, X3S, REFH, true>, nullptr}}
#define X3F_SPLITS(SP) {{x3f_go<SP, false, 3, false, false>, nullptr}, {x3f_go<SP, false, 3, true, false>, nullptr}}
#define X3F_PLANES(SP, NP) {{x3f_go<SP, true, NP, false, false>, x3f_go<SP, true, NP, false, true>}, {x3f_go<SP, true, NP, true, false>, x3f_go<SP, true, NP, true, true>}}
static const AttnEntry attn_table[ATTN_FORMS] = {
    /* ATTN_F32              */ {"attn_kernel<float, false>", ATTN_ROWS(float, false, false, false)},
    /*                       */ {"attn_kernel<float, true>", ATTN_ROWS(float, true, false, false)},
    /* ATTN_F32_QK_X3        */ {"attn_kernel<float, false, x3>", ATTN_ROWS(float, false, true, false)},
    /*                       */ {"attn_kernel<float, true, x3>", ATTN_ROWS(float, true, true, false)},
    /* ATTN_X3F              */ {"attn_x3f_kernel<false>", X3F_SPLITS(false)},
    /*                       */ {"attn_x3f_kernel<true>", X3F_SPLITS(true)},
    /* ATTN_X3F_BF16X3       */ {"attn_x3f_kernel<false, pre-split K V>", X3F_PLANES(false, 3)},
    /*                       */ {"attn_x3f_kernel<true, pre-split K V>", X3F_PLANES(true, 3)},
    /* ATTN_X3F_PAIRS        */ {"attn_x3f_kernel<false, pre-split K V, fp16 pairs>", X3F_PLANES(false, 2)},
    /*                       */ {"attn_x3f_kernel<true, pre-split K V, fp16 pairs>", X3F_PLANES(true, 2)},
    /* ATTN_X3F_PAIRS_SLICED */ {"attn_x3f_kernel<false, pre-split K V, fp16 pairs> + key slices", X3F_PLANES(false, 2)},
    /* ATTN_F16              */ {"attn_kernel<_Float16, false>", ATTN_ROWS(f16, false, false, false)},
    /*                       */ {"attn_kernel<_Float16, true>", ATTN_ROWS(f16, true, false, false)},
    /* ATTN_F16_REF          */ {"attn_kernel<_Float16, false, reference-fp16 scores>", ATTN_ROWS(f16, false, false, true)},
    /*                       */ {"attn_kernel<_Float16, true, reference-fp16 scores>", ATTN_ROWS(f16, true, false, true)},
    /* ATTN_BF16             */ {"attn_kernel<__bf16, false>", ATTN_ROWS(bf16, false, false, false)},
    /*                       */ {"attn_kernel<__bf16, true>", ATTN_ROWS(bf16, true, false, false)},
};
#undef ATTN_ROWS
#undef X3F_SPLITS
#undef X3F_PLANES

AttnPlan attention_plan(int BH, int H, int N, int dtype, bool caller_can_presplit_kv, bool has_lens, float ref_fp16_scale, long ws_floats,
                        long cnt_n) {
    MI_REQUIRE(ref_fp16_scale == 0.f || (dtype == MI_F16 && ref_fp16_scale > 0.f), "attention: the reference-fp16 score form needs f16 operands");
    MI_REQUIRE(H > 0 && BH % H == 0 && N > 0, "attention: bad shape");
    const bool f32 = dtype == MI_F32;
    AttnPlan p;
    p.kv = attention_kv_layout(N, dtype, caller_can_presplit_kv);
    p.varlen = has_lens; p.BH = BH; p.H = H; p.N = N; p.dtype = dtype;
    const int x3 = f32 ? opt_attn_x3() : 0, split = opt(OPT_ATTN_SPLIT);
    p.o_planes = f32 && x3 == 2;
    const int xm = (opt(OPT_ATTN_XCD_MAP) != 0 && BH % 8 == 0) ? 1 : 0;
    const int tiles = (N + ATTN_TILE - 1) / ATTN_TILE, tiles_split = (N + ATTN_TILE_SPLIT - 1) / ATTN_TILE_SPLIT, nstage = (N + ATTN_STAGE - 1) / ATTN_STAGE;
    if (ws_floats <= 0 || cnt_n <= 0) ws_floats = cnt_n = 0;
    // Few 128-query workgroups (fp32: one or two utterances; 16-bit: one — attention 24.3 -> 21.1 ms per step; at two utterances,
    // 576 workgroups, the 128-query form is already balanced and shares each K / V stage among more waves): halve them along the
    // keys, see attn_kernel, and cut the key range into Z slices when that evens out the workgroups per CU.
    const bool small = split && (long)tiles * BH < (f32 ? 1024 : 512) && N >= 64;
    int base, Z = 1;
    if (!f32) {
        base = dtype == MI_BF16 ? ATTN_BF16 : ref_fp16_scale != 0.f ? ATTN_F16_REF : ATTN_F16;
        if (base == ATTN_F16_REF) p.sscale = ref_fp16_scale; else p.xmap = xm;
        if (small) Z = attn_pick_z((long)tiles_split * BH, ATTN_SLOT_SPLIT, nstage, false, std::min((int)opt(OPT_ATTN_Z), (int)opt(OPT_ATTN_Z16)), ws_floats, cnt_n);
    } else {
        base = x3 == 1 ? ATTN_F32_QK_X3 : x3 != 2 ? ATTN_F32 : p.kv.kv_planes == 2 ? ATTN_X3F_PAIRS : p.kv.kv_planes ? ATTN_X3F_BF16X3 : ATTN_X3F;
        if (base == ATTN_X3F_PAIRS) p.xmap = xm;
        // attn_split = 2 (the default for the pre-split fp16-pair kernel, round 4): keep the 128-query workgroups, whose four waves
        // share every K / V stage and multiply two tiles per barrier pair, and cut only the key range into slices: 288 x 3 workgroups
        // for one utterance, 56.3 against 60.0 us per launch on the same box (step 177.8 -> 174.3 ms)
        if (small && base == ATTN_X3F_PAIRS && split == 2) {
            const long units = (long)tiles * BH;
            AttnSlices sl;
            sl.Z = attn_pick_z(units, ATTN_SLOT, nstage, true, opt(OPT_ATTN_Z), ws_floats, cnt_n);
            auto fits = [&](int z) { return units * z * ATTN_SLOT <= ws_floats && units <= cnt_n; };
            if (opt(OPT_ATTN_LPT) && opt(OPT_ATTN_Z_FORCE) == 0 && ws_floats > 0) {      // uneven slices, longest first (attn_pick_slices)
                int zm = std::min((int)opt(OPT_ATTN_Z), ATTN_MAX_SLICES);
                while (zm > 1 && !fits(zm)) --zm;
                sl = attn_pick_slices(units, nstage, 3 * device_cus(), zm);
                if (const AttnCuts& e = opt_attn_cuts(); e.n >= 1 && e.c[0] > 0 && e.c[0] < nstage && fits(e.n + 1)) {      // experiments: MI355TTS_ATTN_CUTS
                    sl.Z = e.n + 1; sl.cut[0] = e.c[0]; sl.cut[1] = e.n >= 2 ? e.c[1] : nstage; sl.cut[2] = e.n >= 3 ? e.c[2] : nstage;
                }
            }
            p.form = ATTN_X3F_PAIRS_SLICED;
            p.grid[0] = tiles; p.grid[1] = BH; p.grid[2] = sl.Z;
            p.cut[0] = sl.Z > 1 ? sl.cut[0] : 0; p.cut[1] = sl.cut[1]; p.cut[2] = sl.cut[2];
            p.label = attn_table[p.form].label;
            return p;
        }
        if (small) Z = attn_pick_z((long)tiles_split * BH, ATTN_SLOT_SPLIT, nstage, true, opt(OPT_ATTN_Z), ws_floats, cnt_n);
    }
    p.form = base + (small ? 1 : 0);
    p.grid[0] = small ? tiles_split : tiles; p.grid[1] = BH; p.grid[2] = Z;
    p.label = attn_table[p.form].label;
    return p;
}

void launch_attention(const AttnPlan& p, const void* q, const void* k, const void* v, void* o, void* o_planes, int o_np, float* ws, int* cnt,
                      const int* lens, hipStream_t s) {
    MI_REQUIRE(p.form >= 0 && p.form < ATTN_FORMS && p.BH > 0, "attention: no plan");
    MI_REQUIRE(o_np == 2 || o_np == 3, "attention: 2 or 3 output planes");
    MI_REQUIRE(!o_planes || p.o_planes, "attention: panel-plane output needs the fp32 split kernel");
    MI_REQUIRE(p.varlen == (lens != nullptr), "attention: the plan was made for a batch of the other kind (uniform / ragged)");
    MI_REQUIRE(p.grid[2] == 1 || (ws && cnt), "attention: the plan's key slices need the workspace it was told of");
    const AttnThunk go = attn_table[p.form].go[p.varlen ? 1 : 0][p.kv.v_rows ? 1 : 0];
    MI_REQUIRE(go, "attention: V as rows is a layout of the pre-split planes");
    const double esz = (double)dtype_size(p.dtype);
    ProfScope ps(FAM_ATTN, s, 4.0 * p.BH * p.N * 64.0 * esz, 4.0 * p.BH * (double)p.N * p.N * 64.0);
    prof_set_kernel(p.label);
    if (lens) prof_kernel_suffix(" + lengths");
    go({p, q, k, v, o, o_planes, o_np, ws, cnt, lens, s});
    MI_HIP(hipGetLastError());
}

}  // namespace mi
