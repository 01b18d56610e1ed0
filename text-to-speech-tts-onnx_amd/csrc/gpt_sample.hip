// gpt_sample.hip — seeded temperature / top-k / top-p sampling of one mel code per sentence slot, inside the decode step
// (and inside its captured hipGraph): the definition is in include/mi355tts.h ("sampling"), this is its device form.
//
// One 1024-thread workgroup per slot, the logits in registers (NPT per thread, code c = tid + j * 1024), no sort:
//   1. z = (logits * pen) * inv_T, block max (and its lowest index: the greedy answer)
//   2. t_k: radix select on order-preserving uint keys, four 8-bit passes over a 256-bin COUNT histogram in LDS
//   3. e = exp(z - max) on K as 2^-40 fixed point (uint64), S = block sum
//   4. t_p: the same descent over MASS-weighted bins (uint64 sums)
//   5. index-order CDF: one uint64 sum per 64 consecutive codes (a wave's row of registers), a scan of those <= 256 sums by
//      wave 0, a wave scan inside the bucket that holds u * S_P
// Histograms are LDS atomics on integers.  Masses are integers and not fp32 so that every sum is independent of the order
// the atomics land in: the chosen token is a pure function of (logits, pen, parameters, n), bit-reproducible between launches,
// slots, batch sizes and graph replays.  exp() underflows to a zero mass 27.7 below the maximum (2^-40); such codes stay
// members of K / P by their key, they just cannot be drawn (their probability is below 1e-12).
#include "gpt_pick.h"

namespace mi {

struct GptSampleShared {
    unsigned long long mass[256];
    unsigned hist[256];
    float wf[16];
    int wi[16];
    unsigned long long wq[16];
    unsigned long long sel_mass, s_p;
    unsigned sel_bin, sel_need;
    int token;
};

template <typename T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The token for decode index n = (n_lo, n_hi) of one row.  Called by all 1024 threads; the result is valid in every thread.
// u_out / prob_out (unit entry only) may be null.
template <int NPT>
__device__ int gpt_sample_token(const float* __restrict__ logits, const float* __restrict__ pen, int codes,
                                const GptSampleRec& r, unsigned n_lo, unsigned n_hi, GptSampleShared& sh,
                                float* __restrict__ u_out, float* __restrict__ prob_out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int top_k = r.top_k;
    const bool greedy = top_k == 1;
    const float inv_T = r.inv_T;
    float z[NPT];
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int c = tid + j * 1024;
        z[j] = -INFINITY;
        if (c < codes) {
            const float v = logits[c] * (pen ? pen[c] : 1.f);
            z[j] = greedy ? v : v * inv_T;
        }
    }
    const unsigned u24 = philox4x32_10(n_lo, n_hi, 0u, 0u, r.seed_lo, r.seed_hi).x >> 8;
    if (u_out && tid == 0) *u_out = (float)u24 * 0x1p-24f;
    if (tid == 0) { sh.sel_bin = 0; sh.sel_need = 1; sh.sel_mass = 1; sh.token = 0; }

    // block max, lowest index on ties (ascending j is ascending c)
    float m = -INFINITY;
    int im = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int c = tid + j * 1024;
        if (c < codes && (z[j] > m || im == 0x7fffffff)) { m = z[j]; im = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(m, o, 64);
        const int oi = __shfl_xor(im, o, 64);
        if (ov > m || (ov == m && oi < im)) { m = ov; im = oi; }
    }
    if (lane == 0) { sh.wf[wave] = m; sh.wi[wave] = im; }
    __syncthreads();
    m = sh.wf[0]; im = sh.wi[0];
#pragma unroll
    for (int q = 1; q < 16; ++q) {
        const float ov = sh.wf[q];
        const int oi = sh.wi[q];
        if (ov > m || (ov == m && oi < im)) { m = ov; im = oi; }
    }
    if (im == 0x7fffffff) im = 0;
    if (greedy) {
        if (prob_out) {
#pragma unroll
            for (int j = 0; j < NPT; ++j) {
                const int c = tid + j * 1024;
                if (c < codes) prob_out[c] = c == im ? 1.f : 0.f;
            }
        }
        return im;
    }

    unsigned key[NPT];
#pragma unroll
    for (int j = 0; j < NPT; ++j) key[j] = order_key(z[j]);

    // ---- top-k: the k-th largest key, with multiplicity --------------------------------------------------------------------
    unsigned tk_key = 0;
    if (top_k > 0 && top_k < codes) {
        unsigned prefix = 0, mask = 0, need = (unsigned)top_k;
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            if (tid < 256) sh.hist[tid] = 0;
            __syncthreads();
#pragma unroll
            for (int j = 0; j < NPT; ++j)
                if (tid + j * 1024 < codes && (key[j] & mask) == prefix) atomicAdd(&sh.hist[(key[j] >> shift) & 255u], 1u);
            __syncthreads();
            if (wave == 0) select_from_top<unsigned>(sh.hist, need, lane, &sh.sel_bin, &sh.sel_need);
            __syncthreads();
            prefix |= sh.sel_bin << shift;
            mask |= 255u << shift;
            need = sh.sel_need;
        }
        tk_key = prefix;
    }

    // ---- e = exp(z - max) on K in 2^-40 fixed point, S -----------------------------------------------------------------------
    unsigned long long q[NPT];
    unsigned long long s = 0;
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const bool in_k = tid + j * 1024 < codes && key[j] >= tk_key;
        q[j] = in_k ? __float2ull_rn(expf(z[j] - m) * 0x1p40f) : 0ull;
        s += q[j];
    }
    s = wave_sum(s);
    if (lane == 0) sh.wq[wave] = s;
    __syncthreads();
    unsigned long long S = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) S += sh.wq[w];

    // ---- top-p: the largest key at which the mass from the top reaches top_p * S -----------------------------------------------
    unsigned tp_key = tk_key;
    if (r.top_p < 1.f) {
        // ceil(top_p * S) in integers (a double product would round once S passes 2^53): top_p = m24 * 2^(ex - 24) exactly,
        // S <= 2^54, so the 128-bit product S * m24 shifted right by rs = 24 - ex >= 24 is exact
        int ex;
        const unsigned long long m24 = (unsigned long long)ldexpf(frexpf(r.top_p, &ex), 24);
        const unsigned long long lo = S * m24, hi = __umul64hi(S, m24);          // hi < 2^14
        const int rs = 24 - ex;
        unsigned long long need;
        if (rs < 64) need = ((hi << (64 - rs)) | (lo >> rs)) + ((lo & ((1ull << rs) - 1ull)) != 0ull);
        else if (rs < 128) need = (hi >> (rs - 64)) + (lo != 0ull || (hi & ((1ull << (rs - 64)) - 1ull)) != 0ull);
        else need = 1ull;
        need = need < 1ull ? 1ull : (need > S ? S : need);
        unsigned prefix = 0, mask = 0;
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            if (tid < 256) sh.mass[tid] = 0;
            __syncthreads();
#pragma unroll
            for (int j = 0; j < NPT; ++j)
                if (q[j] != 0 && (key[j] & mask) == prefix) atomicAdd(&sh.mass[(key[j] >> shift) & 255u], q[j]);
            __syncthreads();
            if (wave == 0) select_from_top<unsigned long long>(sh.mass, need, lane, &sh.sel_bin, &sh.sel_mass);
            __syncthreads();
            prefix |= sh.sel_bin << shift;
            mask |= 255u << shift;
            need = sh.sel_mass;
        }
        tp_key = prefix > tk_key ? prefix : tk_key;
    }

    // ---- the draw: CDF in index order.  Bucket b = j * 16 + wave holds codes 64 b .. 64 b + 63 ---------------------------------
    unsigned in_p = 0;
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const bool p = tid + j * 1024 < codes && key[j] >= tp_key;
        in_p |= (unsigned)p << j;
        if (!p) q[j] = 0;
        unsigned long long bs = 0;
        if (__ballot(q[j] != 0) != 0ull) bs = wave_sum(q[j]);
        if (lane == 0) sh.mass[j * 16 + wave] = bs;
    }
    __syncthreads();
    if (wave == 0) {
        unsigned long long v[4];
        unsigned long long t = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[i] = 4 * lane + i < NPT * 16 ? sh.mass[4 * lane + i] : 0ull; t += v[i]; }
        const unsigned long long incl = wave_incl_scan(t, lane);
        const unsigned long long s_p = __shfl(incl, 63, 64);
        // the token is the first c with cum(c) > u * S_P, u = u24 * 2^-24: cum is an integer, so cum > floor(u24 * S_P / 2^24)
        const unsigned long long thr = (__umul64hi(s_p, (unsigned long long)u24) << 40) | ((s_p * u24) >> 24);
        unsigned long long b = incl - t;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (b <= thr && thr < b + v[i]) { sh.sel_bin = (unsigned)(4 * lane + i); sh.sel_mass = thr - b; }
            b += v[i];
        }
        if (lane == 0) sh.s_p = s_p;
    }
    __syncthreads();
    const unsigned bucket = sh.sel_bin;
    if (wave == (int)(bucket & 15u)) {
        const int jb = (int)(bucket >> 4);
        unsigned long long v = 0;
#pragma unroll
        for (int j = 0; j < NPT; ++j) if (j == jb) v = q[j];
        const unsigned long long incl = wave_incl_scan(v, lane);
        const unsigned long long hit = __ballot(incl > sh.sel_mass);
        if (lane == 0) sh.token = hit ? (int)(bucket * 64u) + __ffsll((long long)hit) - 1 : im;
    }
    __syncthreads();
    if (prob_out) {
        const double inv = 0x1p40 / (double)sh.s_p;
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            const int c = tid + j * 1024;
            if (c < codes) prob_out[c] = (in_p >> j & 1u) ? (float)((double)expf(z[j] - m) * inv) : 0.f;
        }
    }
    return sh.token;
}

template <int NPT>
__global__ __launch_bounds__(1024) void gpt_sample_kernel(const float* __restrict__ logits, float* __restrict__ pen,
                                                          const float* __restrict__ last, int* __restrict__ st,
                                                          int* __restrict__ toks, float* __restrict__ hid, int codes,
                                                          int hidden, int rows, const float* __restrict__ rep_dev, int max_tok,
                                                          const float* __restrict__ emb, const float* __restrict__ pos,
                                                          int max_pos, float* xa, float* xb,
                                                          const GptSampleRec* __restrict__ recs) {
    __shared__ GptSampleShared sh;
    {   // one block per sentence slot
        const size_t sl = blockIdx.x;
        logits += sl * codes; pen += sl * codes; last += sl * hidden; st += sl * GS_WORDS; toks += sl * max_tok;
        hid += sl * (size_t)max_tok * hidden;
        recs += sl;
    }
    GptPickLoads L;
    gpt_pick_load(L, st, rep_dev, toks, last, max_tok, hidden);
    const GptSampleRec r = *recs;
    const int n = st[GS_NDEC];                 // the sentence's decode index: the Philox counter
    const int idx = gpt_sample_token<NPT>(logits, pen, codes, r, (unsigned)n, 0u, sh, nullptr, nullptr);
    gpt_pick_finish(idx, L, pen, st, toks, hid, codes, hidden, rows, max_tok, emb, pos, max_pos, xa, xb);
}

template <int NPT>
__global__ __launch_bounds__(1024) void gpt_sample_rows_kernel(const float* __restrict__ logits, const float* __restrict__ pen,
                                                               int codes, const GptSampleRec* __restrict__ recs,
                                                               const int64_t* __restrict__ positions,
                                                               int32_t* __restrict__ tokens, float* __restrict__ u_out,
                                                               float* __restrict__ prob_out) {
    __shared__ GptSampleShared sh;
    const size_t row = blockIdx.x;
    const GptSampleRec r = recs[row];
    const unsigned long long n = (unsigned long long)positions[row];
    const int idx = gpt_sample_token<NPT>(logits + row * codes, pen ? pen + row * codes : nullptr, codes, r, (unsigned)n,
                                          (unsigned)(n >> 32), sh, u_out + row, prob_out ? prob_out + row * codes : nullptr);
    if (threadIdx.x == 0) tokens[row] = idx;
}

#define GPT_SAMPLE_NPT(codes, CALL)                     \
    do {                                                \
        if ((codes) <= 1024) { CALL(1); }               \
        else if ((codes) <= 4096) { CALL(4); }          \
        else if ((codes) <= 9216) { CALL(9); }          \
        else { CALL(16); }                              \
    } while (0)

void launch_gpt_sample(int nb, const float* logits, float* pen, const float* last, int* st, int* toks, float* hid, int codes,
                       int hidden, int rows, const float* rep_dev, int max_tok, const float* emb, const float* pos, int max_pos,
                       float* xa, float* xb, const GptSampleRec* recs, hipStream_t s) {
    MI_REQUIRE(codes >= 1 && codes <= GPT_SAMPLE_MAX_CODES, "gpt: sampling supports 1..16384 mel codes");
    MI_REQUIRE(nb >= 1 && hidden <= 2048 && recs, "gpt: sampler launch");
#define CALL(N) hipLaunchKernelGGL(gpt_sample_kernel<N>, dim3(nb), dim3(1024), 0, s, logits, pen, last, st, toks, hid, codes, hidden, rows, rep_dev, max_tok, emb, pos, max_pos, xa, xb, recs)
    GPT_SAMPLE_NPT(codes, CALL);
#undef CALL
    MI_HIP(hipGetLastError());
}

void launch_gpt_sample_rows(const float* logits, const float* pen, int rows, int codes, const GptSampleRec* recs,
                            const int64_t* positions, int32_t* tokens, float* u_out, float* prob_out, hipStream_t s) {
    MI_REQUIRE(codes >= 1 && codes <= GPT_SAMPLE_MAX_CODES, "gpt: sampling supports 1..16384 mel codes");
    MI_REQUIRE(rows >= 1 && logits && recs && positions && tokens && u_out, "gpt: sampler launch");
#define CALL(N) hipLaunchKernelGGL(gpt_sample_rows_kernel<N>, dim3(rows), dim3(1024), 0, s, logits, pen, codes, recs, positions, tokens, u_out, prob_out)
    GPT_SAMPLE_NPT(codes, CALL);
#undef CALL
    MI_HIP(hipGetLastError());
}

}  // namespace mi
