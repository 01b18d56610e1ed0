// gpt_pick.h — what the two token-choosing kernels of the IndexTTS decode step share: gpt_pick_kernel (gpt.hip, greedy) and
// gpt_sample_kernel (gpt_sample.hip, temperature / top-k / top-p).  Both are one 1024-thread workgroup per sentence slot;
// they differ only in how the token is chosen from logits * penalty.
#pragma once
#include "gpt.h"

namespace mi {

// per-slot sampling parameters (device array beside the GS_* state; written by the host before a sampled call)
struct GptSampleRec {
    float inv_T;               // 1.0f / temperature, computed on the host in fp32
    float top_p;               // (0, 1]
    int32_t top_k;             // 0 = every code; 1 = greedy (argmax of logits * penalty, no draw)
    uint32_t seed_lo, seed_hi;
    uint32_t pad[3];
};
static_assert(sizeof(GptSampleRec) == 32, "GptSampleRec is 8 words");

constexpr int GPT_SAMPLE_MAX_CODES = 16384;      // 16 logits per thread of a 1024-thread workgroup

// what a pick kernel requests before it looks at the logits (nothing here depends on the choice)
struct GptPickLoads {
    int w[GS_WORDS];           // thread 0: the slot's state words
    float repv;                // thread 0: REPEAT_PENALITY
    int tok_r;                 // thread 0: the oldest penalised token
    float lastv[2];            // every thread: its elements of the last_hidden_state row (hidden <= 2048)
};

__device__ __forceinline__ void gpt_pick_load(GptPickLoads& L, const int* __restrict__ st, const float* __restrict__ rep_dev,
                                              const int* __restrict__ toks, const float* __restrict__ last, int max_tok,
                                              int hidden) {
    const int tid = threadIdx.x;
    L.repv = 0.f;
    L.tok_r = 0;
    if (tid == 0) {
#pragma unroll
        for (int q = 0; q < GS_WORDS; q += 4) {
            const int4 v = *reinterpret_cast<const int4*>(st + q);
            L.w[q] = v.x; L.w[q + 1] = v.y; L.w[q + 2] = v.z; L.w[q + 3] = v.w;
        }
        L.repv = rep_dev[0];
        const int r = L.w[GS_RESET];
        L.tok_r = (r >= 0 && r < max_tok) ? toks[r] : 0;
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) L.lastv[q] = tid + q * 1024 < hidden ? last[tid + q * 1024] : 0.f;
}

// The driver loop's bookkeeping for the chosen token `idx` (valid in thread 0): token store, stop test, penalty update and
// reset over penalty_range, limit, last_hidden_state row, and graph C for the next decode step.  Called by every thread of
// the workgroup (it synchronises).  Pointers are the slot's own.
__device__ __forceinline__ void gpt_pick_finish(int idx, GptPickLoads& L, float* __restrict__ pen, int* __restrict__ st,
                                                int* __restrict__ toks, float* __restrict__ hid, int codes, int hidden, int rows,
                                                int max_tok, const float* __restrict__ emb, const float* __restrict__ pos,
                                                int max_pos, float* xa, float* xb) {
    __shared__ int slot, next_id, next_gen;
    const int tid = threadIdx.x;
    int* w = L.w;
    if (tid == 0) {
        slot = -1;
        if (!w[GS_DONE]) {
            const int t = idx, n = w[GS_NDEC];
            w[GS_TOKEN] = t;
            if (n < max_tok) { toks[n] = t; slot = n; }
            w[GS_NDEC] = n + 1;
            bool stop = false;
#pragma unroll
            for (int q = 0; q < GS_WORDS - GS_STOP0; ++q) stop |= (q < w[GS_NSTOP] && w[GS_STOP0 + q] == t);
            if (stop) w[GS_DONE] = 1;
            else if (w[GS_UPDATE_PEN]) {                      // Inference_IndexTTS_ONNX.py:768-772
                pen[t] = L.repv;          // device scalar: the captured decode graphs must see a changed REPEAT_PENALITY
                const int r = w[GS_RESET];
                // toks[r] was fetched before toks[n] = t above: the same element only if r == n
                const int tr = (r == n && n < max_tok) ? t : L.tok_r;
                if (n + 1 > w[GS_RANGE] && r < max_tok && tr != t) { pen[tr] = 1.f; w[GS_RESET] = r + 1; }
            }
            w[GS_HIST] += rows;
            w[GS_GEN_LEN] += 1;
            if (w[GS_LIMIT] > 0 && n + 1 >= w[GS_LIMIT]) w[GS_DONE] = 1;      // `while num_decode < generate_limit`
#pragma unroll
            for (int q = 0; q < GS_STOP0; q += 4) *reinterpret_cast<int4*>(st + q) = make_int4(w[q], w[q + 1], w[q + 2], w[q + 3]);
            if (GS_STOP0 % 4) { for (int q = GS_STOP0 / 4 * 4; q < GS_STOP0; ++q) st[q] = w[q]; }
        }
        next_id = w[GS_TOKEN]; next_gen = w[GS_GEN_LEN];
    }
    __syncthreads();
    if (slot >= 0) {
#pragma unroll
        for (int q = 0; q < 2; ++q)
            if (tid + q * 1024 < hidden) hid[(size_t)slot * hidden + tid + q * 1024] = L.lastv[q];
    }
    // graph C for the next decode step (IndexTTS_C.forward, Export_IndexTTS.py:222-225) from the state just written:
    // the step's input row, so that a decode step does not start with a launch of its own for it
    const int id = min(max(next_id, 0), codes - 1), g = min(max(next_gen, 0), max_pos - 1);
    for (int c = tid; c < hidden; c += 1024) {
        const float v = emb[(size_t)id * hidden + c] + pos[(size_t)g * hidden + c];
        if (xa) xa[c] = v;
        if (xb) xb[(size_t)blockIdx.x * hidden + c] = v;
    }
}

// ---- shared by the sampler (gpt_sample.hip) and pool-mode beam search (gpt_beam_pool.hip) ------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11): the four output words for counter (c0, c1, c2, c3) and key (k0, k1).  The sampler reads
// word 0 of counter (n, 0, 0, 0); pool-mode beam sampling reads word (i & 3) of counter (n, i >> 2, 1, 0) (gpt_beam_pool.hip)
__device__ __forceinline__ uint4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return make_uint4(c0, c1, c2, c3);
}

// float -> uint whose unsigned order is the float order (-0 and +0 share a key, as they compare equal)
__device__ __forceinline__ unsigned order_key(float z) {
    unsigned b = __float_as_uint(z);
    if (b == 0x80000000u) b = 0;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

template <typename T> __device__ __forceinline__ T wave_incl_scan(T v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}
// wave 0: bins of h[0..256) walked from the top; the bin in which the running sum from above reaches `need`, and what of
// `need` is left for that bin, go to *bin / *rest (and the bin's own total to *cnt)
template <typename T>
__device__ __forceinline__ void select_from_top(const T* h, T need, int lane, unsigned* bin, T* rest, T* cnt = nullptr) {
    T v[4];
    T s = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[i] = h[255 - 4 * lane - i]; s += v[i]; }
    T b = wave_incl_scan(s, lane) - s;                      // everything in bins above this lane's four
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (b < need && need <= b + v[i]) { *bin = (unsigned)(255 - 4 * lane - i); *rest = need - b; if (cnt) *cnt = v[i]; }
        b += v[i];
    }
}

// gpt_sample.hip
// one token per slot by the header's sampling definition (include/mi355tts.h); grid = slots, arguments as gpt_pick_kernel's
void launch_gpt_sample(int nb, const float* logits, float* pen, const float* last, int* st, int* toks, float* hid, int codes,
                       int hidden, int rows, const float* rep_dev, int max_tok, const float* emb, const float* pos, int max_pos,
                       float* xa, float* xb, const GptSampleRec* recs, hipStream_t s);
// the same device code on rows of logits (mi_gpt_sample_logits): device arrays; pen / prob_out may be null
void launch_gpt_sample_rows(const float* logits, const float* pen, int rows, int codes, const GptSampleRec* recs,
                            const int64_t* positions, int32_t* tokens, float* u_out, float* prob_out, hipStream_t s);

}  // namespace mi
