// gpt_prompt.hip — packed prompt pass of the IndexTTS GPT: the prompts of all sentences admitted together run graph E in ONE
// pass over the weights (Gpt::forward_packed), and the per-slot resets a refilled slot needs.
//
// forward_rows (gpt.hip) runs one prompt at a time: k prompts are k passes over every weight matrix, each a GEMM with M ~ 100
// rows.  Here the k prompts lie back to back in X and every LayerNorm / linear layer runs once over all packed rows (the same
// launch_rownorm / launch_conv_gemm path, M = the packed row count).  Only two things know about sentences:
//   * the KV scatter: packed row r of segment g -> cache row r - first_g of slot slot_g (the slot's history is 0);
//   * the attention: work item (head, packed row) finds its segment in a small device table and attends to the keys
//     0 .. rows_g - 1 of its own slot with the reference's additive mask (-128 on keys j > i, every key visited): the prompt
//     attention body of gpt_attn.h, which gpt_attn_kernel (gpt.hip) runs for a lone prompt.  It never reads a cache row
//     beyond rows_g: a refilled slot still holds the rows of the sentence before.
// The tail (ln_f + final_norm + lm_head on each segment's last row, then the token choice) is forward_rows' own, per segment.
// With beams (Gpt::beams != 0) a segment's slot is its group's first slot and the token choice is replaced by selection 0 of all
// the pass's groups in one launch (gpt_beam_first_segs_kernel, gpt_beam.hip, over the same segment table).
#include "gpt.h"
#include "gpt_attn.h"
#include "gpt_pick.h"
#include "gpt_vec.h"
#include "wave_reduce.h"

namespace mi {

// the segment that holds packed row r: segments are ascending and gap-free, so it is the last one that starts at or before r
// (wave-uniform: r comes from blockIdx or is searched per thread over at most GPT_MAX_BATCH = 64 entries)
__device__ __forceinline__ int4 gpt_find_seg(const int4* __restrict__ segs, int nseg, int r) {
    int4 g = segs[0];
    for (int q = 1; q < nseg; ++q) {
        const int4 n = segs[q];
        if (n.x <= r) g = n;
    }
    return g;
}

// rows of (q | k | v) -> K / V cache rows of each row's own slot, one layer (kc / vc = slot 0's layer; slots are slot_stride
// apart).  One 16-byte group per thread.
template <typename T>
__global__ __launch_bounds__(256) void kv_scatter_kernel(const T* __restrict__ qkv, T* __restrict__ kc, T* __restrict__ vc,
                                                         const int4* __restrict__ segs, int nseg, int total, int hidden,
                                                         int max_seq, int max_batch, size_t slot_stride) {
    constexpr int V = Pack16<T>::N;
    const int per = 2 * hidden / V;                        // 16-byte groups of a row's k | v part
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)total * per) return;
    const int r = (int)(i / per), c = (int)(i % per) * V;
    const int4 g = gpt_find_seg(segs, nseg, r);
    const int pos = r - g.x;
    if (pos < 0 || pos >= g.y || pos >= max_seq || g.z < 0 || g.z >= max_batch) return;
    const int which = c / hidden, cc = c % hidden, head = cc >> 6, d = cc & 63;
    const T* src = qkv + (size_t)r * 3 * hidden + hidden + c;
    T* dst = (which ? vc : kc) + (size_t)g.z * slot_stride + ((size_t)head * max_seq + pos) * 64 + d;
    *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
}

// one block per (head, packed row): gpt_prompt_attn_body (gpt_attn.h) over the row's own segment, with the slot, the query
// index and the key count taken from the segment table.  All LDS scratch is in the dynamic region, carved at multiples of
// 16 bytes: sc [max_seq rounded up to 4] | qs [64] | red [8 * 64] | bc [4].
template <typename T>
__global__ __launch_bounds__(512) void gpt_attn_packed_kernel(const T* __restrict__ qkv, const T* __restrict__ kc,
                                                              const T* __restrict__ vc, T* __restrict__ out,
                                                              const int4* __restrict__ segs, int nseg, int hidden,
                                                              int max_seq, int max_batch, size_t slot_stride) {
    extern __shared__ __attribute__((aligned(16))) float psm[];
    float* sc = psm;                           // [max_seq rounded up to 4]
    float* qs = psm + ((max_seq + 3) & ~3);    // [64]
    float* red = qs + 64;                      // [8 * 64]
    float* bc = red + 512;                     // [4]
    const int head = blockIdx.x, row = blockIdx.y;
    const int4 g = gpt_find_seg(segs, nseg, row);
    const int i = row - g.x;                   // the query's position inside its sentence
    const int kv = min(g.y, max_seq);          // keys 0 .. rows_g - 1 of the slot, and no further
    if (i < 0 || i >= kv || g.z < 0 || g.z >= max_batch) return;      // block-uniform: a table that does not cover the row
    kc += (size_t)g.z * slot_stride; vc += (size_t)g.z * slot_stride;
    gpt_prompt_attn_body<T>(i, kv, 1, qkv, kc, vc, out, row, head, hidden, max_seq, sc, qs, red, bc);
}

void launch_gpt_attn_packed(int dtype, const void* qkv, const void* kc, const void* vc, void* out, const void* segs, int nseg,
                            int total, int heads, int hidden, int max_seq, int max_batch, size_t slot_stride, hipStream_t s) {
    const int lds = gpt_packed_attn_lds(max_seq);
#define ATTP(T, ...) hipLaunchKernelGGL(gpt_attn_packed_kernel<T>, dim3(heads, total), dim3(512), lds, s, (const T*)qkv, (const T*)kc, (const T*)vc, (T*)out, (const int4*)segs, nseg, hidden, max_seq, max_batch, slot_stride)
    GPT_DISPATCH(ATTP, 0);
#undef ATTP
}

void gpt_attn_packed_reserve(int lds) {
    MI_HIP(hipFuncSetAttribute((const void*)gpt_attn_packed_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    MI_HIP(hipFuncSetAttribute((const void*)gpt_attn_packed_kernel<f16>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    MI_HIP(hipFuncSetAttribute((const void*)gpt_attn_packed_kernel<bf16>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
}

__global__ __launch_bounds__(256) void gpt_fill_kernel(float* __restrict__ p, float v, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

void Gpt::reset_penalty(int slot) {
    MI_REQUIRE(slot >= 0 && slot < cfg.max_batch, "gpt: penalty slot");
    const int n = cfg.mel_codes;
    hipLaunchKernelGGL(gpt_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       pen.as<float>() + (size_t)slot * n, 1.f, n);
    MI_HIP(hipGetLastError());
}

// Copy-out of a queue session's round: entry q moves tokens and last_hidden_state rows [first, first + count) of slot `slot` to
// rows dst_row .. of the destination arrays (the caller's (n, cap) arrays, or a packed staging buffer).  One block per (row of
// the longest entry, entry); the table travels as a kernel argument, so a round costs one launch and no upload.
__global__ __launch_bounds__(256) void gpt_copy_out_kernel(Gpt::OutTable tab, const int32_t* __restrict__ toks,
                                                           const float* __restrict__ hid, int32_t* __restrict__ tokens_dst,
                                                           float* __restrict__ hidden_dst, int hidden, int max_seq, int max_batch) {
    const Gpt::OutSeg g = tab.e[blockIdx.y];
    const int r = blockIdx.x;
    if (r >= g.count || g.slot < 0 || g.slot >= max_batch || g.first < 0 || g.first + r >= max_seq) return;      // block-uniform
    const size_t src = (size_t)g.slot * max_seq + g.first + r;
    const size_t dst = (size_t)(g.dst_row + r);
    if (tokens_dst && threadIdx.x == 0) tokens_dst[dst] = toks[src];
    if (hidden_dst)
        for (int c = threadIdx.x; c < hidden; c += 256) hidden_dst[dst * hidden + c] = hid[src * hidden + c];
}

void Gpt::copy_out_rows(const OutTable& tab, int n, int32_t* tokens_dst, float* hidden_dst) {
    MI_REQUIRE(n >= 0 && n <= GPT_MAX_BATCH, "gpt: copy-out table");
    int rows = 0;
    for (int q = 0; q < n; ++q) {
        const OutSeg& g = tab.e[q];
        MI_REQUIRE(g.slot >= 0 && g.slot < cfg.max_batch && g.first >= 0 && g.count >= 0 && g.first + g.count <= cfg.max_seq &&
                       g.dst_row >= 0, "gpt: copy-out entry");
        rows = std::max(rows, (int)g.count);
    }
    if (n == 0 || rows == 0 || (!tokens_dst && !hidden_dst)) return;
    hipLaunchKernelGGL(gpt_copy_out_kernel, dim3(rows, n), dim3(256), 0, stream, tab, toks.as<int32_t>(), hid.as<float>(), tokens_dst,
                       hidden_dst, cfg.hidden, cfg.max_seq, cfg.max_batch);
    MI_HIP(hipGetLastError());
}

static_assert(GPT_MAX_BATCH <= 64, "forward_packed keeps the slots of a pass in a 64-bit mask");

void Gpt::forward_packed(const Seg* segs, int k) {
    const GptCfg& c = cfg;
    const int h = c.hidden, S = c.max_seq;
    hipStream_t s = stream;
    const size_t es = dtype_size(dtype);
    MI_REQUIRE(segs && k >= 1 && k <= c.max_batch, "gpt: packed pass segments");
    // beam search: a segment's slot is its group's first slot — the prompt's keys and values are stored once per sentence there
    if (beams) MI_REQUIRE(beams <= GPT_BEAM_MAX && pen_b.p, "gpt: the packed prompt pass of a beam queue needs the beam state");
    int total = 0;
    uint64_t used = 0;                         // one bit per slot (GPT_MAX_BATCH = 64)
    for (int g = 0; g < k; ++g) {
        MI_REQUIRE(segs[g].first == total && segs[g].rows >= 1, "gpt: packed segments must be ascending and gap-free");
        MI_REQUIRE(segs[g].slot >= 0 && segs[g].slot < c.max_batch && !(used >> segs[g].slot & 1u), "gpt: packed segment slot");
        MI_REQUIRE(!beams || (segs[g].slot % beams == 0 && segs[g].slot + beams <= c.max_batch), "gpt: packed segment group");
        used |= (uint64_t)1 << segs[g].slot;
        total += segs[g].rows;
        MI_REQUIRE(total <= S, "gpt: packed rows exceed the prompt scratch (max_seq)");
    }
    if (total == 1) {                          // linear() is the multi-row path: a lone one-row prompt is the single-row pass
        forward_rows(1, 1, segs[0].slot);
        if (beams && pool) pool_select_first(segs[0].slot / beams, beams, 1);
        else if (beams) beam_select_first(segs[0].slot / beams, beams, 1);   // as mi_gpt_generate_beam's one-by-one pass
        return;
    }
    if (!packed_ready) {
        segtab.ensure((size_t)c.max_batch * sizeof(Seg));
        gpt_attn_packed_reserve(gpt_packed_attn_lds(S));
        packed_ready = true;
    }
    static_assert(sizeof(Seg) == sizeof(int4), "Seg is one int4 on the device");
    MI_HIP(hipMemcpyAsync(segtab.p, segs, (size_t)k * sizeof(Seg), hipMemcpyHostToDevice, s));
    MI_HIP(hipStreamSynchronize(s));           // `segs` may be a temporary
    const int4* tab = segtab.as<int4>();
    float* x = X.as<float>();
    const size_t sstride = slot_cache_elems();
    for (int li = 0; li < c.layers; ++li) {
        Layer& l = L[li];
        const LayerKV lc = layer_cache(li);                          // slot 0's layer; slots are slot_cache_elems apart
        char *kcl = lc.k, *vcl = lc.v;
        launch_rownorm(NORM_LN_AFFINE, x, xn.p, dtype, l.ln1_w.as<float>(), l.ln1_b.as<float>(), total, h, 1e-5f, s);
        linear(l.qkv, xn.p, total, qkv.p, dtype, ACT_NONE, nullptr);
        {
            const long items = (long)total * (2 * h / (16 / (int)es));
            const dim3 grid((unsigned)((items + 255) / 256));
#define KVS(T, ...) hipLaunchKernelGGL(kv_scatter_kernel<T>, grid, dim3(256), 0, s, (const T*)qkv.p, (T*)kcl, (T*)vcl, tab, k, total, h, S, c.max_batch, sstride)
            GPT_DISPATCH(KVS, 0);
#undef KVS
        }
        {
            double keys = 0.0;
            for (int g = 0; g < k; ++g) keys += (double)segs[g].rows * segs[g].rows;
            ProfScope ps(FAM_ATTN, s, 2.0 * (double)h * total * es, 4.0 * (double)h * keys);
            launch_gpt_attn_packed(dtype, qkv.p, kcl, vcl, att.p, tab, k, total, c.heads, h, S, c.max_batch, sstride, s);
        }
        linear(l.proj, att.p, total, x, MI_F32, ACT_NONE, x);
        launch_rownorm(NORM_LN_AFFINE, x, xn.p, dtype, l.ln2_w.as<float>(), l.ln2_b.as<float>(), total, h, 1e-5f, s);
        linear(l.fc, xn.p, total, ff.p, dtype, ACT_GELU_TANH, nullptr);
        linear(l.fc2, ff.p, total, x, MI_F32, ACT_NONE, x);
    }
    for (int g = 0; g < k; ++g) {
        const int slot = segs[g].slot;
        const float* xl = x + (size_t)(segs[g].first + segs[g].rows - 1) * h;
        // ln_f (-> last_hidden_state) and final_norm in front of the lm_head, one launch, as in forward_rows
        gemv(head, xl, fn_w.as<float>(), fn_b.as<float>(), logits.as<float>() + (size_t)slot * c.mel_codes, MI_F32, ACT_NONE,
             nullptr, nullptr, nullptr, 0, lnf_w.as<float>(), lnf_b.as<float>(), last.as<float>() + (size_t)slot * h);
        // X still holds the other segments' rows: the token's graph C goes to the slot's batched decode row only
        if (!beams) choose_token(segs[g].rows, slot, false);
    }
    // beam search: selection 0 of all admitted groups from the segment table the pass left on the device, one launch
    // (pool mode: the pool-mode selection, gpt_beam_pool.hip)
    if (beams && pool) pool_select_segs(k, beams);
    else if (beams) beam_select_segs(k, beams);
}

}  // namespace mi
