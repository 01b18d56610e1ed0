// gpt_lin.h — device helpers shared by the decode-step linear kernels of gpt.hip (16-bit / fp32 weights) and gpt_q8.hip
// (per-channel uint8 weights): the activation, the non-temporal 16-byte load, the multi-value wave reduction, the matrix-core
// wrapper and the epilogue of a skinny tile.
#pragma once
#include "gpt.h"
#include "gpt_attn.h"
#include "gpt_vec.h"
#include "mfma.h"

namespace mi {

__device__ inline float gelu_new(float x) {
    return 0.5f * x * (1.f + tanhf(0.7978845608028654f * (x + 0.044715f * x * x * x)));
}

#ifndef GPT_NT
#define GPT_NT 1
#endif
#if GPT_NT
#define GPT_WLOAD ldnt16
#else
#define GPT_WLOAD ld16
#endif
template <typename T> __device__ inline Pack16<T> ldnt16(const T* p) {
    Pack16<T> r;
    *reinterpret_cast<u32x4*>(&r) = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    return r;
}

// NV per-lane partial sums -> full sums: after the call, lane l holds the total of value index
//   idx = sum_s ((l >> (5 - s)) & 1) << (log2(NV) - 1 - s)   (and every lane sharing those bits holds the same total).
// log2(NV) halving exchange steps (NV - 1 shuffles) + the remaining butterfly, instead of 6 * NV shuffles.
template <int NV> __device__ inline float reduce_multi(float (&v)[NV], int lane) {
    int off = 32;
#pragma unroll
    for (int n = NV; n > 1; n >>= 1) {
        const bool hi = (lane & off) != 0;
#pragma unroll
        for (int i = 0; i < n / 2; ++i) {
            const float send = hi ? v[i] : v[i + n / 2];
            const float keep = hi ? v[i + n / 2] : v[i];
            v[i] = keep + __shfl_xor(send, off, 64);
        }
        off >>= 1;
    }
    for (; off > 0; off >>= 1) v[0] += __shfl_xor(v[0], off, 64);
    return v[0];
}

constexpr int GB_KC = 1024;       // K chunk of the batched GEMV kernels: the x rows of a chunk are shared through LDS

typedef float f32x4_t __attribute__((ext_vector_type(4)));
template <typename T> struct Mfma16;
template <> struct Mfma16<f16> {
    using Frag = f16x8;
    static __device__ __forceinline__ f32x4_t mma(Frag a, Frag b, f32x4_t c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};
template <> struct Mfma16<bf16> {
    using Frag = bf16x8;
    static __device__ __forceinline__ f32x4_t mma(Frag a, Frag b, f32x4_t c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};

// epilogue of one lane's four D values of a skinny tile: rows n4 .. n4+3 of sentence b (bias, activation, residual; QKV: the
// k / v rows go to cache row st[b].hist of slot b)
template <typename T, bool QKV>
__device__ __forceinline__ void skinny_store(f32x4_t acc, int b, int n4, const float* __restrict__ bias, const float* res,
                                             void* out, int out_f32, int act, int N, T* __restrict__ kc, T* __restrict__ vc,
                                             const int* __restrict__ st, int max_seq, size_t slot_stride) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int n = n4 + r;
        if (n >= N) continue;
        float v = acc[r] + (bias ? bias[n] : 0.f);
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

}  // namespace mi
