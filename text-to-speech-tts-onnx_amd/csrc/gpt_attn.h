// gpt_attn.h — the two attention bodies of the IndexTTS GPT, and the cache address of the decode linears' QKV epilogues.
//
//   gpt_attn1_body         decode step (one new row, no mask): gpt_attn1_kernel (gpt.hip, every row in the block's own slot)
//                          and gpt_attn1_beam_kernel (gpt_beam.hip, rows found through the ancestor table) differ only in
//                          the row locator they pass.
//   gpt_prompt_attn_body   prompt rows (additive mask): gpt_attn_kernel (gpt.hip) and gpt_attn_packed_kernel
//                          (gpt_prompt.hip) differ only in how they find the slot, the query index, the key count and
//                          their LDS carve-up.
// The kernels keep their own argument lists and prologues; the bodies are force-inlined into them.
#pragma once
#include "gpt.h"
#include "gpt_vec.h"
#include "wave_reduce.h"

namespace mi {

// element offset of column `col` (head = col >> 6) of cache row `pos` inside one layer's [head][max_seq][64] block
__device__ __forceinline__ size_t kv_cache_offset(int col, int pos, int max_seq) {
    return ((size_t)(col >> 6) * max_seq + pos) * 64 + (col & 63);
}

// Row locators of gpt_attn1_body: which slot's cache (counted from the kb / vb the body is given) holds a row.
//   key_slot(j)            the slot of key j, asked by the lane that holds that key
//   value_slot(sl, src)    the slot of the value row whose key sits in lane `src` of this pass (sl = this lane's key_slot)
//   offset(slot)           that slot's distance in elements
// direct: always the block's own slot, no load
struct AttnRowsOwn {
    __device__ __forceinline__ int key_slot(int) const { return 0; }
    __device__ __forceinline__ int value_slot(int, int) const { return 0; }
    __device__ __forceinline__ size_t offset(int) const { return 0; }
};
// ancestor (beam search): position P + n of the hypothesis lives in slot anc[n] of its group, the prompt's rows below P in
// the group's first slot.  One extra dependent load per lane and pass, in front of the K loads.
struct AttnRowsAncestor {
    const int* anc;
    int P, B, max_seq;
    size_t slot_stride;
    __device__ __forceinline__ int key_slot(int j) const {
        // branch-free: the table is read at a clamped index and the answer dropped for prompt rows; a wrong entry can only
        // name another slot of the group
        const int a = anc[min(max(j - P, 0), max_seq - 1)];
        return j >= P ? min(max(a, 0), B - 1) : 0;
    }
    __device__ __forceinline__ int value_slot(int sl, int src) const { return __shfl(sl, src, 64); }
    __device__ __forceinline__ size_t offset(int slot) const { return (size_t)slot * slot_stride; }
};

// Decode-step attention of row `slot` of qkv / out for one head, called by a block of 4 waves: kc / vc = this layer's cache
// of the slot the locator counts from, kv = keys.  Each wave owns every fourth 64-key pass and
// runs its own online softmax (lane = key for the scores, 16-byte K loads against the packed q; the pass's V rows are
// fetched before the softmax so their latency overlaps it), so the block needs ONE barrier: the four (max, sum, O)
// partials meet in LDS at the end.
template <typename T, typename Rows>
__device__ __forceinline__ void gpt_attn1_body(const T* qkv, const T* kc, const T* vc, T* out, int slot, int head, int hidden,
                                               int max_seq, int kv, const Rows& rows) {
    constexpr int V = Pack16<T>::N;            // elements per 16 bytes
    constexpr int CH = 64 / V;                 // 16-byte chunks per 64-wide row
    constexpr int KPI = 64 / CH;               // value rows per wave instruction
    constexpr int NIT = 64 / KPI;              // instructions per 64-key pass
    __shared__ float part[4][66];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Pack16<T> q[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) q[c] = ld16(qkv + (size_t)slot * 3 * hidden + head * 64 + c * V);
    const T* kb = kc + (size_t)head * max_seq * 64;
    const T* vb = vc + (size_t)head * max_seq * 64;
    const int g = lane / CH, c = lane % CH;
    float m_run = -INFINITY, l_run = 0.f, acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = 0.f;
    struct Pass { Pack16<T> kp[CH], vp[NIT]; };
    auto load_pass = [&](Pass& ps, int base) {
        const int j = base + lane;
        const int jc = j < kv ? j : base;
        const int sl = rows.key_slot(jc);
        const T* kr = kb + rows.offset(sl) + (size_t)jc * 64;
#pragma unroll
        for (int cc = 0; cc < CH; ++cc) ps.kp[cc] = ld16(kr + cc * V);
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int jj = base + it * KPI + g;
            const bool ok = jj < kv;
            const int sv = rows.value_slot(sl, ok ? it * KPI + g : 0);
            ps.vp[it] = ld16(vb + rows.offset(sv) + (size_t)(ok ? jj : base) * 64 + c * V);
        }
    };
    auto fold_pass = [&](const Pass& ps, int base) {
        const bool kok = base + lane < kv;
        float s = 0.f;
#pragma unroll
        for (int cc = 0; cc < CH; ++cc) s = dot_pack(ps.kp[cc], q[cc], s);
        s = kok ? s : -INFINITY;
        const float mw = wave_max(s);
        const float m_new = fmaxf(m_run, mw);              // finite: the pass holds at least one key
        const float pj = kok ? __expf(s - m_new) : 0.f;
        const float corr = __expf(m_run - m_new);          // exp(-inf) = 0 on the first pass
        l_run = l_run * corr + wave_sum(pj);
        m_run = m_new;
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] *= corr;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const float pk = __shfl(pj, it * KPI + g, 64);  // 0 for keys beyond kv
#pragma unroll
            for (int e = 0; e < V; ++e) acc[e] = fmaf(pk, (float)ps.vp[it].v[e], acc[e]);
        }
    };
    // the wave's passes (every fourth 64-key block), the next one in flight while the current one is folded in
    int base = wave * 64;
    if (base < kv) {
        Pass pa, pb;
        load_pass(pa, base);
        for (;;) {
            bool more = base + 256 < kv;
            if (more) load_pass(pb, base + 256);
            fold_pass(pa, base);
            if (!more) break;
            base += 256;
            more = base + 256 < kv;
            if (more) load_pass(pa, base + 256);
            fold_pass(pb, base);
            if (!more) break;
            base += 256;
        }
    }
#pragma unroll
    for (int o = CH; o < 64; o <<= 1)
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] += __shfl_xor(acc[e], o, 64);
    if (lane == 0) { part[wave][0] = m_run; part[wave][1] = l_run; }
    if (g == 0)
#pragma unroll
        for (int e = 0; e < V; ++e) part[wave][2 + c * V + e] = acc[e];
    __syncthreads();
    if (wave == 0) {
        float M = part[0][0];
#pragma unroll
        for (int w = 1; w < 4; ++w) M = fmaxf(M, part[w][0]);
        float L = 0.f, o = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float f = __expf(part[w][0] - M);        // waves without keys: exp(-inf) = 0
            L = fmaf(part[w][1], f, L);
            o = fmaf(part[w][2 + lane], f, o);
        }
        out[(size_t)slot * hidden + head * 64 + lane] = (T)(o / L);
    }
}

// Prompt attention of row `row` of qkv / out for one head, called by a block of 8 waves: softmax(q K^T + mask) V over keys
// 0 .. kv-1 of the slot's layer cache kc / vc for the query at position i.  Scores into LDS, max, exp-sum, value pass, 8-wave merge: lane-per-key dot products (each
// lane streams one 64-wide key row with 16-byte loads; keys beyond 512 come round again in the strided loop), then 8 lanes
// per value row.  LDS: sc [kv] | qs [64] | red [8 * 64] | bc [2], carved by the caller.
template <typename T>
__device__ __forceinline__ void gpt_prompt_attn_body(int i, int kv, int masked, const T* qkv, const T* kc, const T* vc, T* out,
                                                     int row, int head, int hidden, int max_seq, float* sc, float* qs,
                                                     float* red, float* bc) {
    constexpr int V = Pack16<T>::N;            // elements per 16 bytes
    constexpr int CH = 64 / V;                 // 16-byte chunks per key row
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 64) qs[tid] = (float)qkv[(size_t)row * 3 * hidden + head * 64 + tid];
    __syncthreads();
    const T* kb = kc + (size_t)head * max_seq * 64;
    const T* vb = vc + (size_t)head * max_seq * 64;
    float mx = -3.0e38f;
    for (int j = tid; j < kv; j += 512) {
        const T* kr = kb + (size_t)j * 64;
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const Pack16<T> p = ld16(kr + c * V);
#pragma unroll
            for (int e = 0; e < V; ++e) s = fmaf(qs[c * V + e], (float)p.v[e], s);
        }
        if (masked && j > i) s += -128.f;      // the reference's additive mask: not -inf, and no key is skipped
        sc[j] = s;
        mx = fmaxf(mx, s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    if (tid == 0) { float m = red[0]; for (int w = 1; w < 8; ++w) m = fmaxf(m, red[w]); bc[0] = m; }
    __syncthreads();
    mx = bc[0];
    float sum = 0.f;
    for (int j = tid; j < kv; j += 512) { const float e = __expf(sc[j] - mx); sc[j] = e; sum += e; }
    sum = wave_sum(sum);
    __syncthreads();
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    if (tid == 0) { float t = 0.f; for (int w = 0; w < 8; ++w) t += red[w]; bc[1] = t; }
    __syncthreads();
    const float inv = 1.f / bc[1];
    // values: lane = (key-in-group g, chunk c) ; a wave covers 64/CH keys per pass
    constexpr int KPW = 64 / CH;               // keys per wave pass
    const int g = lane / CH, c = lane % CH;
    float acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = 0.f;
    for (int j = wave * KPW + g; j < kv; j += 8 * KPW) {
        const float p = sc[j];
        const Pack16<T> v = ld16(vb + (size_t)j * 64 + c * V);
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = fmaf(p, (float)v.v[e], acc[e]);
    }
    // reduce over g (lanes that share c): xor over the g bits
#pragma unroll
    for (int o = CH; o < 64; o <<= 1)
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] += __shfl_xor(acc[e], o, 64);
    __syncthreads();
    if (g == 0)
#pragma unroll
        for (int e = 0; e < V; ++e) red[wave * 64 + c * V + e] = acc[e];
    __syncthreads();
    if (tid < 64) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) t += red[w * 64 + tid];
        out[(size_t)row * hidden + head * 64 + tid] = (T)(t * inv);
    }
}

}  // namespace mi
