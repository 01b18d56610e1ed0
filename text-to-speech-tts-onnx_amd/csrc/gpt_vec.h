// gpt_vec.h — 16-byte packs and their dot products, shared by the decode kernels of gpt.hip and gpt_beam.hip.
#pragma once
#include "common.h"

namespace mi {

template <typename T> struct Pack16 {
    static constexpr int N = 16 / sizeof(T);
    T v[N];
};
template <typename T> __device__ inline Pack16<T> ld16(const T* p) {
    Pack16<T> r;
    *reinterpret_cast<uint4*>(&r) = *reinterpret_cast<const uint4*>(p);
    return r;
}
// acc += dot(a[0..V), b[0..V)) with fp32 accumulation; 16-bit types use the packed dot instructions (v_dot2_f32_f16 /
// v_dot2_f32_bf16: two multiply-adds per lane per issue, no conversions)
__device__ inline float dot_pack(const Pack16<float>& a, const Pack16<float>& b, float acc) {
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = fmaf(a.v[e], b.v[e], acc);
    return acc;
}
__device__ inline float dot_pack(const Pack16<f16>& a, const Pack16<f16>& b, float acc) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2* pa = reinterpret_cast<const h2*>(&a);
    const h2* pb = reinterpret_cast<const h2*>(&b);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_fdot2(pa[e], pb[e], acc, false);
    return acc;
}
__device__ inline float dot_pack(const Pack16<bf16>& a, const Pack16<bf16>& b, float acc) {
    typedef __bf16 b2 __attribute__((ext_vector_type(2)));
    const b2* pa = reinterpret_cast<const b2*>(&a);
    const b2* pb = reinterpret_cast<const b2*>(&b);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_fdot2_f32_bf16(pa[e], pb[e], acc, false);
    return acc;
}

}  // namespace mi
