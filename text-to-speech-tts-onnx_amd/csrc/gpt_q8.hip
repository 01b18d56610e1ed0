// gpt_q8.hip — the decode-step linears of the IndexTTS GPT on per-channel uint8 weights, dequantised in the kernels.
//
// The format (include/mi355tts.h, mi_gpt_quantize_u8): row n of an (n, k) matrix is bytes q[n, :] with one fp32 scale and one
// uint8 zero point, w ~ float(q - zp) * scale.  It restates the weight side of the reference's int8 export
// (IndexTTS/Optimize_ONNX.py: quantize_dynamic(per_channel=True, weight_type=QUInt8, MatMulConstBOnly=True)); the activations
// stay 16-bit here.  Every kernel computes
//     out[n] = act(scale[n] * sum_k (q[n, k] - zp[n]) * x'[k] + bias[n]) (+ res[n])
// with (q - zp) formed exactly, the sum in fp32 and the scale applied once to the finished sum.  x', the epilogues, the QKV
// cache writes and pre_out are those of the 16-bit kernels of gpt.hip, whose structure these kernels keep: one 16-byte
// non-temporal load is 16 weights of a row, every global load of a block is issued before the first reduction (x-side
// operands first), rows at or beyond nb are never written.
//
// How the bytes become operands:
//   * gemv_d_q8_kernel (one sentence, fp32 FMAs): v_cvt_f32_ubyte, minus float(zp);
//   * gemv_b_q8_kernel (v_dot2_f32_f16) and the two matrix-core kernels: the halfword 0x6400 | byte is the f16 number
//     1024 + byte, and (1024 + byte) - (1024 + zp) is exact in f16 (integers up to 2048 are), so two packed f16 subtractions turn
//     four bytes into four exact (q - zp) operands.
// The 16-bit prompt pass (rows > 1) reads a dequantised copy of the matrix it is about to use (gpt_dequant_q8_kernel into a scratch
// the handle owns), through the unchanged implicit-GEMM path.
//
// Activations are f16: bf16 has no such byte form, and the handle refuses it (mi_gpt_create_q8).
#include "gpt.h"
#include "gpt_attn.h"
#include "gpt_vec.h"
#include "gpt_lin.h"
#include "mfma.h"
#include "lds_dma.h"         // buf_rsrc
#include "wave_reduce.h"
#include "options.h"
#include <cmath>

namespace mi {

// ---------------------------------------------------------------------------------------------------------------
// host quantiser (no HIP call)
// ---------------------------------------------------------------------------------------------------------------
void gpt_quantize_u8(const float* w, int n, int k, uint8_t* q, float* scale, uint8_t* zp) {
    for (int r = 0; r < n; ++r) {
        const float* row = w + (size_t)r * k;
        float rmin = 0.f, rmax = 0.f;
        for (int c = 0; c < k; ++c) { rmin = std::min(rmin, row[c]); rmax = std::max(rmax, row[c]); }
        float sc = (rmax - rmin) / 255.f, z = 0.f;
        if (rmax == rmin) sc = 1.f;                        // an all-zero row
        else z = std::min(255.f, std::max(0.f, std::nearbyintf(-rmin / sc)));      // round half to even
        scale[r] = sc;
        zp[r] = (uint8_t)z;
        uint8_t* qr = q + (size_t)r * k;
        for (int c = 0; c < k; ++c)
            qr[c] = (uint8_t)std::min(255.f, std::max(0.f, std::nearbyintf(row[c] / sc) + z));
    }
}

// ---------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------
typedef _Float16 h2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u32x4 q8_load(const uint8_t* p) {
    return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
}
// bytes 0, 1 / 2, 3 of a word as the f16 pair (1024 + byte): the byte under the exponent pattern 0x64
__device__ __forceinline__ h2_t q8_pair_lo(uint32_t w) { return __builtin_bit_cast(h2_t, (w & 0xffu) | ((w & 0xff00u) << 8) | 0x64006400u); }
__device__ __forceinline__ h2_t q8_pair_hi(uint32_t w) { return __builtin_bit_cast(h2_t, ((w >> 16) & 0xffu) | ((w >> 8) & 0xff0000u) | 0x64006400u); }
// eight bytes -> eight exact (q - zp) in f16; off = (1024 + zp) in both halves
__device__ __forceinline__ f16x8 q8_frag(uint32_t w0, uint32_t w1, h2_t off) {
    const h2_t a = q8_pair_lo(w0) - off, b = q8_pair_hi(w0) - off, c = q8_pair_lo(w1) - off, d = q8_pair_hi(w1) - off;
    return f16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}
__device__ __forceinline__ h2_t q8_off(int zp) { const _Float16 o = (_Float16)(1024 + zp); return h2_t{o, o}; }
__device__ __forceinline__ float q8_dot8(f16x8 a, const Pack16<f16>& x, float acc) {
    const h2_t* px = reinterpret_cast<const h2_t*>(&x);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_fdot2(h2_t{a[2 * e], a[2 * e + 1]}, px[e], acc, false);
    return acc;
}

// gemv_d_kernel (gpt.hip) on uint8 weight rows: lane l holds k = 16 l + 1024 it .. + 16 of the row, KI = ceil(K / 1024).
template <typename T, int R, int KI, int WAVES, bool LN, bool QKV>
__global__ __launch_bounds__(WAVES * 64) void gemv_d_q8_kernel(const uint8_t* __restrict__ w, const float* __restrict__ scale,
                                                               const uint8_t* __restrict__ zp, const void* __restrict__ xin,
                                                               const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                                               const float* __restrict__ pre_w, const float* __restrict__ pre_b,
                                                               float* __restrict__ pre_out,
                                                               const float* __restrict__ bias, const float* res, void* out,
                                                               int out_f32, int act, int N, int K, T* __restrict__ kc,
                                                               T* __restrict__ vc, const int* __restrict__ st, int max_seq) {
    constexpr int V = 16;                                 // weights per 16-byte load
    constexpr int VT = Pack16<T>::N;                      // activations per 16 bytes
    constexpr int KP = KI * 64 * V;                       // padded K
    constexpr int XI = (KP / VT + WAVES * 64 - 1) / (WAVES * 64);      // 16-byte x loads per thread (plain form)
    __shared__ __attribute__((aligned(16))) float xs[LN ? KP : 4];
    __shared__ __attribute__((aligned(16))) T xt[LN ? 8 : XI * WAVES * 64 * VT];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n0 = (blockIdx.x * WAVES + wave) * R;
    // epilogue operands of the row this lane will store (lane r < R) and the rows' zero points, fetched up front
    const int nrow = min(n0 + (lane < R ? lane : 0), N - 1);
    const float bias_pre = bias ? bias[nrow] : 0.f;
    const float res_pre = res ? res[nrow] : 0.f;
    const float scale_pre = scale[nrow];
    const int pos_pre = QKV ? st[GS_HIST] : 0;
    float zpf[R];
#pragma unroll
    for (int r = 0; r < R; ++r) zpf[r] = (float)zp[min(n0 + r, N - 1)];
    u32x4 p[KI][R];
    auto load_weights = [&]() {
#pragma unroll
    for (int it = 0; it < KI; ++it) {
        const int k = lane * V + it * 64 * V;
#pragma unroll
        for (int r = 0; r < R; ++r)         // branch-free: padded lanes re-read k = 0 of the row and meet x = 0 in LDS
            p[it][r] = q8_load(w + (size_t)min(n0 + r, N - 1) * K + (k < K ? k : 0));
    }
    };
    if constexpr (LN) {
        const float* xf = (const float*)xin;
        if (pre_w) {      // rownorm_kernel<float, 8>, NORM_LN_AFFINE, one wave per row: here wave 0 (as gemv_d_kernel)
            if (wave == 0) {
                constexpr int MAXV = 8;
                float4 v[MAXV];
                float s = 0.f;
#pragma unroll
                for (int i = 0; i < MAXV; ++i) {
                    const int c = (i * 64 + lane) * 4;
                    v[i] = c < K ? *reinterpret_cast<const float4*>(xf + c) : make_float4(0, 0, 0, 0);
                    s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
                }
                const float mean = wave_sum(s) / (float)K;
                float q = 0.f;
#pragma unroll
                for (int i = 0; i < MAXV; ++i) {
                    const int c = (i * 64 + lane) * 4;
                    if (c < K) {
                        const float d0 = v[i].x - mean, d1 = v[i].y - mean, d2 = v[i].z - mean, d3 = v[i].w - mean;
                        q += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
                    }
                }
                const float inv = 1.0f / sqrtf(wave_sum(q) / (float)K + 1e-5f);
#pragma unroll
                for (int i = 0; i < MAXV; ++i) {
                    const int c = (i * 64 + lane) * 4;
                    if (c < K) {
                        const float4 av = *reinterpret_cast<const float4*>(pre_w + c);
                        const float4 bv = *reinterpret_cast<const float4*>(pre_b + c);
                        float o[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
                        const float aa[4] = {av.x, av.y, av.z, av.w}, bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
                        for (int k = 0; k < 4; ++k) { const float n = (o[k] - mean) * inv; o[k] = n * aa[k] + bb[k]; }
                        const float4 ov = make_float4(o[0], o[1], o[2], o[3]);
                        *reinterpret_cast<float4*>(&xs[c]) = ov;
                        if (blockIdx.x == 0 && pre_out) *reinterpret_cast<float4*>(pre_out + c) = ov;
                    }
                }
            }
            __syncthreads();
        }
        float xe[KI][V];
#pragma unroll
        for (int it = 0; it < KI; ++it) {
            const int k = lane * V + it * 64 * V;
            const bool ok = k < K;
            const int kk = ok ? k : 0;
#pragma unroll
            for (int e = 0; e < V; e += 4) {
                float4 v;
                if (pre_w) v = *reinterpret_cast<const float4*>(&xs[kk + e]);      // uniform branch
                else v = *reinterpret_cast<const float4*>(xf + kk + e);
                xe[it][e] = ok ? v.x : 0.f; xe[it][e + 1] = ok ? v.y : 0.f; xe[it][e + 2] = ok ? v.z : 0.f; xe[it][e + 3] = ok ? v.w : 0.f;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // gamma / beta of the (iteration, 4-element group) items this wave turns into LayerNorm(x); then the weights
        constexpr int QV = V / 4, NITEM = KI * QV, MYI = (NITEM + WAVES - 1) / WAVES;
        float4 gq[MYI], bq[MYI];
#pragma unroll
        for (int m = 0; m < MYI; ++m) {
            const int item = wave + m * WAVES;
            const int k = lane * V + (item / QV) * 64 * V + (item % QV) * 4;
            const int kk = item < NITEM && k < K ? k : 0;
            gq[m] = *reinterpret_cast<const float4*>(ln_w + kk);
            bq[m] = *reinterpret_cast<const float4*>(ln_b + kk);
        }
        __builtin_amdgcn_sched_barrier(0);
        load_weights();
        __builtin_amdgcn_sched_barrier(0);
        float sum = 0.f;
#pragma unroll
        for (int it = 0; it < KI; ++it)
#pragma unroll
            for (int e = 0; e < V; ++e) sum += xe[it][e];
        const float mean = wave_sum(sum) / (float)K;
        float sq = 0.f;
#pragma unroll
        for (int it = 0; it < KI; ++it) {
            const bool ok = lane * V + it * 64 * V < K;
#pragma unroll
            for (int e = 0; e < V; ++e) { const float d = ok ? xe[it][e] - mean : 0.f; sq = fmaf(d, d, sq); }
        }
        const float rstd = rsqrtf(wave_sum(sq) / (float)K + 1e-5f);
        if (pre_w) __syncthreads();                       // every wave holds its share of the ln_f row: xs is reused
#pragma unroll
        for (int item = 0; item < NITEM; ++item) {
            if (item % WAVES == wave) {
                const int it = item / QV, q = item % QV, m = item / WAVES;
                const int k = lane * V + it * 64 * V + q * 4;
                float4 o = make_float4(0, 0, 0, 0);
                if (k < K) {
                    const float4 g = gq[m], b = bq[m];
                    o.x = (xe[it][q * 4 + 0] - mean) * rstd * g.x + b.x;
                    o.y = (xe[it][q * 4 + 1] - mean) * rstd * g.y + b.y;
                    o.z = (xe[it][q * 4 + 2] - mean) * rstd * g.z + b.z;
                    o.w = (xe[it][q * 4 + 3] - mean) * rstd * g.w + b.w;
                }
                *reinterpret_cast<float4*>(&xs[k]) = o;
            }
        }
        __syncthreads();
    } else {
        const T* xr = (const T*)xin;
        u32x4 xv[XI];                                      // bounds-checked buffer loads: 0 beyond K, no branch
        const __amdgpu_buffer_rsrc_t rsx = buf_rsrc(xr, K * (int)sizeof(T));
#pragma unroll
        for (int i = 0; i < XI; ++i)
            xv[i] = __builtin_amdgcn_raw_buffer_load_b128(rsx, (int)((threadIdx.x + i * WAVES * 64) * 16), 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        load_weights();
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < XI; ++i) *reinterpret_cast<u32x4*>(&xt[(threadIdx.x + i * WAVES * 64) * VT]) = xv[i];
        __syncthreads();
    }
    float acc[R];                                         // rows beyond N: computed on clamped rows, never stored
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
#pragma unroll
    for (int it = 0; it < KI; ++it) {
        const int k = lane * V + it * 64 * V;
        float xn[V];
        if constexpr (LN) {
#pragma unroll
            for (int e = 0; e < V; e += 4) {
                const float4 v = *reinterpret_cast<const float4*>(&xs[k + e]);
                xn[e] = v.x; xn[e + 1] = v.y; xn[e + 2] = v.z; xn[e + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int h = 0; h < V / VT; ++h) {
                const Pack16<T> xv = ld16(&xt[k + h * VT]);
#pragma unroll
                for (int e = 0; e < VT; ++e) xn[h * VT + e] = (float)xv.v[e];
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float wq = (float)((p[it][r][e >> 2] >> (8 * (e & 3))) & 0xffu) - zpf[r];      // exact
                acc[r] = fmaf(wq, xn[e], acc[r]);
            }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = wave_sum(acc[r]);
    if (lane < R && n0 + lane < N) {
        const int n = n0 + lane;
        float v = acc[0];
#pragma unroll
        for (int r = 1; r < R; ++r) v = lane == r ? acc[r] : v;
        v = v * scale_pre + bias_pre;
        if (act == ACT_GELU_TANH) v = gelu_new(v);
        v += res_pre;
        if (QKV) {
            const int hidden = N / 3;
            if (n >= hidden) {
                const int c = n - hidden, which = c / hidden, cc = c % hidden;
                if (pos_pre < max_seq) (which ? vc : kc)[kv_cache_offset(cc, pos_pre, max_seq)] = (T)v;
                return;
            }
        }
        if (out_f32) ((float*)out)[n] = v; else ((T*)out)[n] = (T)v;
    }
}

// gemv_b_kernel (gpt.hip) on uint8 weight rows: one 16-byte load per row covers a lane's share of a 1024-element K chunk.
template <typename T, int R, int BB, bool QKV>
__global__ __launch_bounds__(512) void gemv_b_q8_kernel(const uint8_t* __restrict__ w, const float* __restrict__ scale,
                                                        const uint8_t* __restrict__ zp, const T* __restrict__ x,
                                                        const float* __restrict__ bias, const float* res, void* out,
                                                        int out_f32, int act, int N, int K, int nb, T* __restrict__ kc,
                                                        T* __restrict__ vc, const int* __restrict__ st, int max_seq,
                                                        size_t slot_stride) {
    static_assert(sizeof(T) == 2 && GB_KC == 64 * 16, "one 16-byte weight load per lane and chunk");
    constexpr int VT = Pack16<T>::N;
    __shared__ __attribute__((aligned(16))) T xs[BB * GB_KC];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n0 = (blockIdx.x * 8 + wave) * R;
    const uint8_t* wr[R];
    h2_t off[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int row = min(n0 + r, N - 1);
        wr[r] = w + (size_t)row * K;
        off[r] = q8_off(zp[row]);
    }
    float acc[R][BB];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int b = 0; b < BB; ++b) acc[r][b] = 0.f;
    const int kl = lane * 16;
    for (int k0 = 0; k0 < K; k0 += GB_KC) {
        const int kn = min(GB_KC, K - k0);
        u32x4 p[R];
#pragma unroll
        for (int r = 0; r < R; ++r) p[r] = q8_load(wr[r] + k0 + (kl < kn ? kl : 0));
        __syncthreads();                            // the previous chunk has been consumed
        for (int i = threadIdx.x * VT; i < BB * kn; i += 512 * VT) {
            const int b = i / kn, kk = i % kn;      // kn is a multiple of 16
            *reinterpret_cast<uint4*>(&xs[b * GB_KC + kk]) = *reinterpret_cast<const uint4*>(x + (size_t)b * K + k0 + kk);
        }
        __syncthreads();
        if (kl < kn) {
            f16x8 wq[R][2];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                wq[r][0] = q8_frag(p[r][0], p[r][1], off[r]);
                wq[r][1] = q8_frag(p[r][2], p[r][3], off[r]);
            }
#pragma unroll
            for (int b = 0; b < BB; ++b) {
                const Pack16<T> x0 = ld16(&xs[b * GB_KC + kl]), x1 = ld16(&xs[b * GB_KC + kl + 8]);
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r][b] = q8_dot8(wq[r][1], x1, q8_dot8(wq[r][0], x0, acc[r][b]));
            }
        }
    }
    if (n0 >= N) return;
    // lane -> slot index it ends up holding (see reduce_multi)
    constexpr int LOG = BB == 16 ? 4 : BB == 8 ? 3 : BB == 4 ? 2 : BB == 2 ? 1 : 0;
    int b = 0;
#pragma unroll
    for (int s = 0; s < LOG; ++s) b |= ((lane >> (5 - s)) & 1) << (LOG - 1 - s);
    const bool writer = (lane & ((64 >> LOG) - 1)) == 0 && b < nb;
    float tot[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float tmp[BB];
#pragma unroll
        for (int q = 0; q < BB; ++q) tmp[q] = acc[r][q];
        tot[r] = reduce_multi<BB>(tmp, lane);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int n = n0 + r;
        if (writer && n < N) {
            float v = tot[r] * scale[n] + (bias ? bias[n] : 0.f);
            if (act == ACT_GELU_TANH) v = gelu_new(v);
            if (res) v += res[(size_t)b * N + n];
            bool to_cache = false;
            if (QKV) {
                const int hidden = N / 3;
                if (n >= hidden) {
                    const int c = n - hidden, which = c / hidden, cc = c % hidden;
                    const int pos = st[b * GS_WORDS + GS_HIST];
                    if (pos < max_seq)
                        (which ? vc : kc)[(size_t)b * slot_stride + kv_cache_offset(cc, pos, max_seq)] = (T)v;
                    to_cache = true;
                }
            }
            if (!to_cache) {
                if (out_f32) ((float*)out)[(size_t)b * N + n] = v; else ((T*)out)[(size_t)b * N + n] = (T)v;
            }
        }
    }
}

// The matrix-core kernels of gpt.hip on uint8 weight rows.  The lane map is theirs: within each 64-wide K block lane group
// g = lane >> 4 takes k = 16g .. 16g + 15 of both operands, which for the weights is ONE 16-byte load that becomes the two A
// fragments of the block; the MFMAs, their order, the KS split and the order of the partial adds are unchanged.  The D rows'
// scales multiply the finished sums in front of the shared epilogue.
__device__ __forceinline__ f32x4_t q8_scaled(f32x4_t acc, const float (&sc)[4]) {
    return f32x4_t{acc[0] * sc[0], acc[1] * sc[1], acc[2] * sc[2], acc[3] * sc[3]};
}

template <typename T, bool QKV, int UNR>
__global__ __launch_bounds__(512) void gemm_skinny_q8_kernel(const uint8_t* __restrict__ w, const float* __restrict__ scale,
                                                             const uint8_t* __restrict__ zp, const T* __restrict__ x,
                                                             const float* __restrict__ bias, const float* res, void* out,
                                                             int out_f32, int act, int N, int K, int nb, int KS,
                                                             T* __restrict__ kc, T* __restrict__ vc,
                                                             const int* __restrict__ st, int max_seq, size_t slot_stride) {
    using MF = Mfma16<T>;
    using Frag = typename MF::Frag;
    __shared__ __attribute__((aligned(16))) float red[8][256];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    const int TR = 8 / KS, tile = wave / KS, ks = wave - tile * KS;
    const int n0 = (blockIdx.x * TR + tile) * 16;
    const int kw = K / KS;
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    float sc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) sc[r] = scale[min(n0 + 4 * g + r, N - 1)];
    if (n0 < N) {
        const int row = min(n0 + i, N - 1);
        const h2_t off = q8_off(zp[row]);
        const uint8_t* wr = w + (size_t)row * K + ks * kw + g * 16;
        const T* xr = x + (size_t)min(i, nb - 1) * K + ks * kw + g * 16;
        // UNR 64-wide K blocks per trip: all 3 * UNR loads are issued before the first MFMA, the x side first
        for (int kb = 0; kb < kw; kb += 64 * UNR) {
            u32x4 a[UNR];
            Frag bq[2 * UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                bq[2 * u] = *reinterpret_cast<const Frag*>(xr + kb + 64 * u);
                bq[2 * u + 1] = *reinterpret_cast<const Frag*>(xr + kb + 64 * u + 8);
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) a[u] = q8_load(wr + kb + 64 * u);
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                acc = MF::mma(q8_frag(a[u][0], a[u][1], off), bq[2 * u], acc);
                acc = MF::mma(q8_frag(a[u][2], a[u][3], off), bq[2 * u + 1], acc);
            }
        }
    }
    *reinterpret_cast<f32x4_t*>(&red[wave][lane * 4]) = acc;
    __syncthreads();
    if (ks != 0 || n0 >= N) return;
    for (int q = 1; q < KS; ++q) {
        const f32x4_t o = *reinterpret_cast<const f32x4_t*>(&red[wave + q][lane * 4]);
        acc += o;
    }
    const int b = i;                                    // D layout: column = lane & 15 (sentence), rows 4*(lane>>4) + r
    if (b >= nb) return;
    skinny_store<T, QKV>(q8_scaled(acc, sc), b, n0 + 4 * g, bias, res, out, out_f32, act, N, kc, vc, st, max_seq, slot_stride);
}

// 17..64 sentences: CT column tiles over one pass of the weight rows; column c is bit for bit column c % 16 of
// gemm_skinny_q8_kernel run on sentences 16 * (c / 16) ... (the same MFMAs in the same order per accumulator, the same partial adds)
template <typename T, bool QKV, int UNR, int CT>
__global__ __launch_bounds__(512) void gemm_skinny_wide_q8_kernel(const uint8_t* __restrict__ w, const float* __restrict__ scale,
                                                                  const uint8_t* __restrict__ zp, const T* __restrict__ x,
                                                                  const float* __restrict__ bias, const float* res, void* out,
                                                                  int out_f32, int act, int N, int K, int nb, int KS,
                                                                  T* __restrict__ kc, T* __restrict__ vc,
                                                                  const int* __restrict__ st, int max_seq, size_t slot_stride) {
    using MF = Mfma16<T>;
    using Frag = typename MF::Frag;
    __shared__ __attribute__((aligned(16))) float red[CT][8][256];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    const int TR = (int)(blockDim.x >> 6) / KS, tile = wave / KS, ks = wave - tile * KS;      // KS waves per 16-row tile
    const int n0 = (blockIdx.x * TR + tile) * 16;
    const int kw = K / KS;
    f32x4_t acc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[c] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float sc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) sc[r] = scale[min(n0 + 4 * g + r, N - 1)];
    if (n0 < N) {
        const int row = min(n0 + i, N - 1);
        const h2_t off = q8_off(zp[row]);
        const uint8_t* wr = w + (size_t)row * K + ks * kw + g * 16;
        const T* xr[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) xr[c] = x + (size_t)min(16 * c + i, nb - 1) * K + ks * kw + g * 16;
        for (int kb = 0; kb < kw; kb += 64 * UNR) {
            u32x4 a[UNR];
            Frag bq[CT][2 * UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u)
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    bq[c][2 * u] = *reinterpret_cast<const Frag*>(xr[c] + kb + 64 * u);
                    bq[c][2 * u + 1] = *reinterpret_cast<const Frag*>(xr[c] + kb + 64 * u + 8);
                }
#pragma unroll
            for (int u = 0; u < UNR; ++u) a[u] = q8_load(wr + kb + 64 * u);
            __builtin_amdgcn_sched_barrier(0);
            // per accumulator the chain runs over u ascending, as in gemm_skinny_q8_kernel; the CT chains interleave
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const Frag a0 = q8_frag(a[u][0], a[u][1], off), a1 = q8_frag(a[u][2], a[u][3], off);
#pragma unroll
                for (int c = 0; c < CT; ++c) acc[c] = MF::mma(a0, bq[c][2 * u], acc[c]);
#pragma unroll
                for (int c = 0; c < CT; ++c) acc[c] = MF::mma(a1, bq[c][2 * u + 1], acc[c]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int c = 0; c < CT; ++c) *reinterpret_cast<f32x4_t*>(&red[c][wave][lane * 4]) = acc[c];
    __syncthreads();
    if (ks != 0 || n0 >= N) return;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        for (int q = 1; q < KS; ++q) {
            const f32x4_t o = *reinterpret_cast<const f32x4_t*>(&red[c][wave + q][lane * 4]);
            acc[c] += o;
        }
        const int b = 16 * c + i;                       // D layout: column = lane & 15 of tile c, rows 4*(lane>>4) + r
        if (b < nb)
            skinny_store<T, QKV>(q8_scaled(acc[c], sc), b, n0 + 4 * g, bias, res, out, out_f32, act, N, kc, vc, st, max_seq, slot_stride);
    }
}

// (n, k) uint8 rows -> T(float(q - zp) * scale): what a 16-bit engine stores when given the dequantised blob.  16 weights per thread.
template <typename T>
__global__ __launch_bounds__(256) void gpt_dequant_q8_kernel(const uint8_t* __restrict__ q, const float* __restrict__ scale,
                                                             const uint8_t* __restrict__ zp, T* __restrict__ out, int n, int k) {
    const long per = k / 16, i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)n * per) return;
    const int row = (int)(i / per);
    const size_t e0 = (size_t)i * 16;
    const u32x4 v = *reinterpret_cast<const u32x4*>(q + e0);
    const float sc = scale[row], z = (float)zp[row];
    Pack16<T> o[2];
#pragma unroll
    for (int e = 0; e < 16; ++e)
        o[e / 8].v[e % 8] = (T)(((float)((v[e >> 2] >> (8 * (e & 3))) & 0xffu) - z) * sc);
    *reinterpret_cast<uint4*>(out + e0) = *reinterpret_cast<const uint4*>(&o[0]);
    *reinterpret_cast<uint4*>(out + e0 + 8) = *reinterpret_cast<const uint4*>(&o[1]);
}

// ---------------------------------------------------------------------------------------------------------------
// launchers (called by launch_gpt_gemv / launch_gpt_gemv_b / launch_gpt_gemv_b16 of gpt.hip when l.wfmt == GPT_W_Q8)
// ---------------------------------------------------------------------------------------------------------------
static void q8_require(const GptLin& l, const char* who) {
    MI_REQUIRE(l.wfmt == GPT_W_Q8 && l.w && l.scale && l.zp, std::string(who) + ": uint8 weights need their scales and zero points");
    MI_REQUIRE(l.dtype == MI_F16, std::string(who) + ": uint8 weights run with MI_F16 activations");
    MI_REQUIRE(l.k % 16 == 0, std::string(who) + ": K must be a multiple of 16 with uint8 weights");
}

template <typename T, int R, int KI, bool LN, bool QKV>
static void gemv_d_q8_launch(const GptLin& l, const void* x, const float* ln_w, const float* ln_b, const float* pre_w,
                             const float* pre_b, float* pre_out, const float* res, void* out, int of, int act, void* kcl,
                             void* vcl, const int* st, int max_seq, hipStream_t s) {
    constexpr int WAVES = LN ? 8 : 4;
    const dim3 grid((unsigned)((l.n + WAVES * R - 1) / (WAVES * R)));
    if (prof_mask()) {      // the template-id as a kernel trace prints it
        char nm[96];
        std::snprintf(nm, sizeof nm, "gemv_d_q8_kernel<%s, %d, %d, %d, %s, %s>", type_label<T>(), R, KI, WAVES, LN ? "true" : "false",
                      QKV ? "true" : "false");
        prof_set_kernel(nm);
    }
    hipLaunchKernelGGL((gemv_d_q8_kernel<T, R, KI, WAVES, LN, QKV>), grid, dim3(WAVES * 64), 0, s, (const uint8_t*)l.w, l.scale, l.zp,
                       x, ln_w, ln_b, pre_w, pre_b, pre_out, l.bias, res, out, of, act, l.n, l.k, (T*)kcl, (T*)vcl, st, max_seq);
}

void launch_gpt_gemv_q8(const GptLin& l, const void* x, const float* ln_w, const float* ln_b, const float* pre_w, const float* pre_b,
                        float* pre_out, void* out, int odt, int act, const float* res, void* kcl, void* vcl, const int* st,
                        int max_seq, hipStream_t s) {
    q8_require(l, "gemv");
    const int of = odt == MI_F32;
    MI_REQUIRE(of || odt == l.dtype, "gemv: output dtype");
    MI_REQUIRE(!kcl || ln_w, "gemv: the QKV epilogue comes with the fused LayerNorm");
    MI_REQUIRE(!ln_w || !res, "gemv: the fused-LayerNorm variant has no residual input");
    MI_REQUIRE(!pre_w || ln_w, "gemv: the leading LayerNorm comes with the fused one");
    ProfScope ps(FAM_CONV_GEMM, s, (double)l.n * l.k, 2.0 * l.n * l.k);
    using T = f16;
    const int ki = (l.k + 1023) / 1024;
#define GD(RR, KK, LNN, QK) gemv_d_q8_launch<T, RR, KK, LNN, QK>(l, x, ln_w, ln_b, pre_w, pre_b, pre_out, res, out, of, act, kcl, vcl, st, max_seq, s)
    if (ln_w) {
        // the normalised row lives in LDS as fp32, 4 iterations of 64 lanes x 16 elements
        MI_REQUIRE(ki <= 4, "gemv: the fused LayerNorm supports K <= 4096 with uint8 weights (4 x 64 lanes x 16 elements)");
        MI_REQUIRE(!pre_w || l.k <= 2048, "gemv: the leading LayerNorm supports K <= 2048 (8 float4 per lane of one wave)");
        const int cus = device_cus();      // rows per wave: as gemv_d_dispatch (gpt.hip)
        int r = 1;
        while (r < (kcl ? 2 : 5) && (l.n + 8 * r - 1) / (8 * r) > cus) ++r;
#define GD_K(RR, QK)                                                                              \
    do {                                                                                          \
        if (ki <= 1) GD(RR, 1, true, QK); else if (ki == 2) GD(RR, 2, true, QK);                   \
        else if (ki == 3) GD(RR, 3, true, QK); else GD(RR, 4, true, QK);                           \
    } while (0)
        if (kcl) { if (r == 2) GD_K(2, true); else GD_K(1, true); }
        else { if (r == 1) GD_K(1, false); else if (r == 2) GD_K(2, false); else if (r == 3) GD_K(3, false); else if (r == 4) GD_K(4, false); else GD_K(5, false); }
#undef GD_K
    } else {
        MI_REQUIRE(ki <= 8, "gemv: K <= 8192");
        if (ki <= 1) GD(1, 1, false, false); else if (ki == 2) GD(1, 2, false, false);
        else if (ki == 3) GD(1, 3, false, false); else if (ki == 4) GD(1, 4, false, false);
        else if (ki == 5) GD(1, 5, false, false); else if (ki == 6) GD(1, 6, false, false);
        else GD(1, 8, false, false);
    }
#undef GD
    MI_HIP(hipGetLastError());
}

// the KS split of the matrix-core kernels and whether K takes it (as gpt.hip)
static inline int q8_ks(int k) { return k > 2048 ? 8 : 4; }
static inline bool q8_mfma(const GptLin& l, int nb) {
    return opt(OPT_GPT_MFMA) && nb >= opt(OPT_GPT_MFMA_MIN) && l.k % (q8_ks(l.k) * 64) == 0;
}

bool launch_gpt_gemv_wide_q8(const GptLin& l, const void* x, int nb, void* out, int of, int act, const float* res, void* kcl,
                             void* vcl, const int* st, int max_seq, size_t sstride, hipStream_t stream) {
    q8_require(l, "gemv_b");
    MI_REQUIRE(nb > 16 && nb <= GPT_MAX_BATCH, "gemv_b: the wide kernel takes 17..64 rows");
    if (!q8_mfma(l, nb)) return false;
    using T = f16;
    const int KS = q8_ks(l.k);
    ProfScope ps(FAM_CONV_GEMM, stream, (double)l.n * l.k, 2.0 * l.n * l.k * nb);
    const int CT = (nb + 15) / 16;
    const int TR = KS == 4 && (l.n + 15) / 16 <= device_cus() ? 1 : 8 / KS;      // one tile per block while that is one round (gpt.hip)
    const dim3 gs((unsigned)((l.n + 16 * TR - 1) / (16 * TR)));
    const bool u5 = (l.k / KS) % 320 == 0;
#define GW1(QK, U, C) do { prof_set_kernel("gemm_skinny_wide_q8_kernel<T, " #QK ", " #U ", " #C ">", type_label<T>()); hipLaunchKernelGGL((gemm_skinny_wide_q8_kernel<T, QK, U, C>), gs, dim3(64 * KS * TR), 0, stream, (const uint8_t*)l.w, l.scale, l.zp, (const T*)x, l.bias, res, out, of, act, l.n, l.k, nb, KS, (T*)kcl, (T*)vcl, st, max_seq, sstride); } while (0)
#define GW2(QK, U) do { if (CT == 2) GW1(QK, U, 2); else if (CT == 3) GW1(QK, U, 3); else GW1(QK, U, 4); } while (0)
#define GW(QK) do { if (u5) GW2(QK, 5); else GW2(QK, 1); } while (0)
    if (kcl) GW(true); else GW(false);
#undef GW
#undef GW2
#undef GW1
    MI_HIP(hipGetLastError());
    return true;
}

void launch_gpt_gemv_b16_q8(const GptLin& l, const void* x, int nb, void* out, int of, int act, const float* res, void* kcl, void* vcl,
                            const int* st, int max_seq, size_t sstride, hipStream_t stream) {
    q8_require(l, "gemv_b");
    MI_REQUIRE(nb >= 1 && nb <= 16, "gemv_b: up to 16 rows");
    using T = f16;
    const int BB = nb <= 2 ? 2 : nb <= 4 ? 4 : nb <= 8 ? 8 : 16;
    const int R = l.n >= 4096 ? 2 : 1;
    ProfScope ps(FAM_CONV_GEMM, stream, (double)l.n * l.k, 2.0 * l.n * l.k * nb);
    if (q8_mfma(l, nb)) {
        const int KS = q8_ks(l.k), TR = 8 / KS;
        const dim3 gs((unsigned)((l.n + 16 * TR - 1) / (16 * TR)));
        const bool u5 = (l.k / KS) % 320 == 0;
#define GS1(QK, U) do { prof_set_kernel("gemm_skinny_q8_kernel<T, " #QK ", " #U ">", type_label<T>()); hipLaunchKernelGGL((gemm_skinny_q8_kernel<T, QK, U>), gs, dim3(512), 0, stream, (const uint8_t*)l.w, l.scale, l.zp, (const T*)x, l.bias, res, out, of, act, l.n, l.k, nb, KS, (T*)kcl, (T*)vcl, st, max_seq, sstride); } while (0)
#define GS(QK) do { if (u5) GS1(QK, 5); else GS1(QK, 1); } while (0)
        if (kcl) GS(true); else GS(false);
#undef GS
#undef GS1
        MI_HIP(hipGetLastError());
        return;
    }
    const dim3 grid((unsigned)((l.n + 8 * R - 1) / (8 * R)));
#define GB(RR, B_, QK) do { prof_set_kernel("gemv_b_q8_kernel<T, " #RR ", " #B_ ", " #QK ">", type_label<T>()); hipLaunchKernelGGL((gemv_b_q8_kernel<T, RR, B_, QK>), grid, dim3(512), 0, stream, (const uint8_t*)l.w, l.scale, l.zp, (const T*)x, l.bias, res, out, of, act, l.n, l.k, nb, (T*)kcl, (T*)vcl, st, max_seq, sstride); } while (0)
#define GB_B(RR, QK) do { if (BB == 2) GB(RR, 2, QK); else if (BB == 4) GB(RR, 4, QK); else if (BB == 8) GB(RR, 8, QK); else GB(RR, 16, QK); } while (0)
    if (kcl) { if (R == 2) GB_B(2, true); else GB_B(1, true); }
    else { if (R == 2) GB_B(2, false); else GB_B(1, false); }
#undef GB_B
#undef GB
    MI_HIP(hipGetLastError());
}

void launch_gpt_dequant_q8(const GptLin& l, void* out, hipStream_t s) {
    q8_require(l, "dequantise");
    const long items = (long)l.n * (l.k / 16);
    hipLaunchKernelGGL(gpt_dequant_q8_kernel<f16>, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, (const uint8_t*)l.w, l.scale,
                       l.zp, (f16*)out, l.n, l.k);
    MI_HIP(hipGetLastError());
}

}  // namespace mi
