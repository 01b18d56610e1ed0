// gpt_beam.hip — beam search of the IndexTTS decode loop on the device: the definition is in include/mi355tts.h ("beam search"),
// this is its device form.  A sentence's B hypotheses sit in B consecutive slots (a group) and every decode step is the batched
// step (Gpt::decode_rows_eager, gpt.h) over nb * B rows with its own attention launch and its own last kernel:
//
//   gpt_beam_step_kernel    one 1024-thread workgroup per sentence, like the two pick kernels: row max and lse of the B rows of
//                           logits * penalty, the B best of the B * codes candidates, then the hypotheses move to their new slots —
//                           penalty vector, GS_* words, score and ancestor table follow the parent; gpt_pick_finish's bookkeeping
//                           with the hypothesis' own token; graph C rows for the next step.
//   gpt_attn1_beam_kernel   the decode-step attention body (gpt_attn1_body, gpt_attn.h) with the slot of every key / value row
//                           taken from the ancestor table: the cache is never copied.  Position P + n of hypothesis i lives in
//                           slot anc[i][n], positions below P (the prompt) in the group's first slot.  The body is the one
//                           gpt_attn1_kernel runs on a privately owned cache, so in fp32 the two outputs are equal.
//
// The move is not in place (two children may share a parent, a child's slot may be another child's parent): penalty vectors and
// ancestor tables exist twice and the side in use is GS_NDEC & 1, read on the device, so a captured step replays unchanged.
// State words and scores are small: the workgroup reads all of them before it writes any.
#include "gpt.h"
#include "gpt_attn.h"
#include "gpt_pick.h"
#include "gpt_vec.h"
#include "wave_reduce.h"

namespace mi {

struct BeamShared {
    float red[16][GPT_BEAM_MAX];
    float rv[2][16];
    int ri[2][16];
    int parent[GPT_BEAM_MAX], code[GPT_BEAM_MAX];
    float score[GPT_BEAM_MAX];
};

constexpr int BEAM_NONE = 0x7fffffff;

__device__ __forceinline__ bool beam_better(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }

// One selection of a group.  lg / pen: the group's first row of logits / penalties (pen may be null = ones), rows `codes` apart;
// prev: the B scores so far (LDS).  first: selection 0, only row 0 is read.  Called by all 1024 threads; parent / code / score of
// the B new hypotheses are left in sh, visible to every thread on return.
__device__ void beam_choose(const float* __restrict__ lg, const float* __restrict__ pen, const float* prev, int B, int codes,
                            int first, BeamShared& sh) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = first ? 1 : B;
    // z = logits * pen: one rounded multiply wherever it is formed (never contracted into the subtraction that follows)
    auto zval = [&](int b, int c) {
        const size_t i = (size_t)b * codes + c;
        return __fmul_rn(lg[i], pen ? pen[i] : 1.f);
    };
    float m[GPT_BEAM_MAX], lse[GPT_BEAM_MAX];
#pragma unroll
    for (int b = 0; b < GPT_BEAM_MAX; ++b) m[b] = -INFINITY;
    for (int c = tid; c < codes; c += 1024) {
#pragma unroll
        for (int b = 0; b < GPT_BEAM_MAX; ++b)
            if (b < R) m[b] = fmaxf(m[b], zval(b, c));
    }
#pragma unroll
    for (int b = 0; b < GPT_BEAM_MAX; ++b) {
        if (b < R) {
            const float w = wave_max(m[b]);
            if (lane == 0) sh.red[wave][b] = w;
        }
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < GPT_BEAM_MAX; ++b) {
        if (b < R) {
            float t = sh.red[0][b];
#pragma unroll
            for (int q = 1; q < 16; ++q) t = fmaxf(t, sh.red[q][b]);
            m[b] = t;
        }
    }
    __syncthreads();
    // sum exp(z - m): ascending codes inside a thread, the wave's fixed tree, the 16 waves in order
    float s[GPT_BEAM_MAX];
#pragma unroll
    for (int b = 0; b < GPT_BEAM_MAX; ++b) s[b] = 0.f;
    for (int c = tid; c < codes; c += 1024) {
#pragma unroll
        for (int b = 0; b < GPT_BEAM_MAX; ++b)
            if (b < R) s[b] += expf(zval(b, c) - m[b]);
    }
#pragma unroll
    for (int b = 0; b < GPT_BEAM_MAX; ++b) {
        if (b < R) {
            const float w = wave_sum(s[b]);
            if (lane == 0) sh.red[wave][b] = w;
        }
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < GPT_BEAM_MAX; ++b) {
        lse[b] = 0.f;
        if (b < R) {
            float t = 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) t += sh.red[q][b];
            lse[b] = m[b] + logf(t);
        }
    }
    // the thread's own B best candidates, best first (B == 1 orders by z itself: greedy does not pass through lse)
    const bool greedy = B == 1;
    float lv[GPT_BEAM_MAX];
    int li[GPT_BEAM_MAX];
#pragma unroll
    for (int q = 0; q < GPT_BEAM_MAX; ++q) { lv[q] = -INFINITY; li[q] = BEAM_NONE; }
#pragma unroll
    for (int b = 0; b < GPT_BEAM_MAX; ++b) {
        if (b < R) {
            const float base = first ? 0.f : prev[b];
            for (int c = tid; c < codes; c += 1024) {
                const float z = zval(b, c);
                float kv = greedy ? z : (first ? z - lse[b] : base + (z - lse[b]));
                int ki = b * codes + c;
#pragma unroll
                for (int q = 0; q < GPT_BEAM_MAX; ++q) {
                    const bool up = beam_better(kv, ki, lv[q], li[q]);
                    const float tv = up ? lv[q] : kv;
                    const int ti = up ? li[q] : ki;
                    lv[q] = up ? kv : lv[q];
                    li[q] = up ? ki : li[q];
                    kv = tv; ki = ti;
                }
            }
        }
    }
    // B rounds of a block-wide best-of-heads; the thread that owned the winner moves its list up
    for (int r = 0; r < B; ++r) {
        float v = lv[0];
        int i = li[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(v, o, 64);
            const int oi = __shfl_xor(i, o, 64);
            if (beam_better(ov, oi, v, i)) { v = ov; i = oi; }
        }
        if (lane == 0) { sh.rv[r & 1][wave] = v; sh.ri[r & 1][wave] = i; }
        __syncthreads();
        v = sh.rv[r & 1][0]; i = sh.ri[r & 1][0];
#pragma unroll
        for (int q = 1; q < 16; ++q) {
            const float ov = sh.rv[r & 1][q];
            const int oi = sh.ri[r & 1][q];
            if (beam_better(ov, oi, v, i)) { v = ov; i = oi; }
        }
        if (i != BEAM_NONE && li[0] == i) {
#pragma unroll
            for (int q = 0; q + 1 < GPT_BEAM_MAX; ++q) { lv[q] = lv[q + 1]; li[q] = li[q + 1]; }
            lv[GPT_BEAM_MAX - 1] = -INFINITY; li[GPT_BEAM_MAX - 1] = BEAM_NONE;
        }
        if (tid == 0) {
            const int flat = i == BEAM_NONE ? 0 : i;       // no candidate compares (every value NaN): code 0 of row 0
            sh.parent[r] = flat / codes;
            sh.code[r] = flat % codes;
            sh.score[r] = greedy ? (first ? v - lse[0] : prev[0] + (v - lse[0])) : v;
        }
    }
    __syncthreads();
}

// mi_gpt_beam_select: one workgroup per group of B rows
__global__ __launch_bounds__(1024) void gpt_beam_select_rows_kernel(const float* __restrict__ logits, const float* __restrict__ pen,
                                                                    const float* __restrict__ prev, int B, int codes, int first,
                                                                    int32_t* __restrict__ parents, int32_t* __restrict__ tokens,
                                                                    float* __restrict__ scores) {
    __shared__ BeamShared sh;
    __shared__ float osc[GPT_BEAM_MAX];
    const size_t row0 = (size_t)blockIdx.x * B;
    if (threadIdx.x < B) osc[threadIdx.x] = first ? 0.f : prev[row0 + threadIdx.x];
    __syncthreads();
    beam_choose(logits + row0 * codes, pen ? pen + row0 * codes : nullptr, osc, B, codes, first, sh);
    if (threadIdx.x < B) {
        parents[row0 + threadIdx.x] = sh.parent[threadIdx.x];
        tokens[row0 + threadIdx.x] = sh.code[threadIdx.x];
        scores[row0 + threadIdx.x] = sh.score[threadIdx.x];
    }
}

// One selection of the group whose first slot is s0, by the whole workgroup: the body of the two kernels below.  pen0 / pen1 and
// anc0 / anc1 are the two sides of what moves with a hypothesis; the side read is GS_NDEC & 1, the other one is written.  rows =
// new cache rows of the forward pass before (the prompt's for selection 0, else 1).  Every index that comes out of memory is
// clamped before it forms an address.
__device__ __forceinline__ void beam_step_body(const float* __restrict__ logits, float* pen0, float* pen1,
                                               const float* __restrict__ last, int* st, int* toks, float* __restrict__ hid,
                                               int* anc0, int* anc1, float* scores, int codes, int hidden, int rows,
                                               const float* __restrict__ rep_dev, int max_tok, const float* __restrict__ emb,
                                               const float* __restrict__ pos, int max_pos, float* __restrict__ xb, int B,
                                               int first, size_t s0) {
    __shared__ BeamShared sh;
    __shared__ int sw[GPT_BEAM_MAX][GS_WORDS];
    __shared__ float osc[GPT_BEAM_MAX];
    __shared__ int pw_t[GPT_BEAM_MAX], pw_r[GPT_BEAM_MAX], new_reset[GPT_BEAM_MAX], s_done;
    const int tid = threadIdx.x;
    if (tid < B * GS_WORDS) sw[tid / GS_WORDS][tid % GS_WORDS] = st[s0 * GS_WORDS + tid];
    if (tid < B) osc[tid] = scores[s0 + tid];
    const float repv = rep_dev[0];
    __syncthreads();
    if (sw[0][GS_DONE]) return;                                    // the sentence is done: the step is a no-op (uniform)
    const int n = sw[0][GS_NDEC];
    const float* pen_old = ((n & 1) ? pen1 : pen0) + s0 * codes;
    float* pen_new = ((n & 1) ? pen0 : pen1) + s0 * codes;
    const int* anc_old = ((n & 1) ? anc1 : anc0) + s0 * max_tok;
    int* anc_new = ((n & 1) ? anc0 : anc1) + s0 * max_tok;
    beam_choose(logits + s0 * codes, pen_old, osc, B, codes, first, sh);
    if (tid < B) {
        const int i = tid, p = min(max(sh.parent[i], 0), B - 1), t = min(max(sh.code[i], 0), codes - 1);
        const int* w = sw[p];
        if (n >= 0 && n < max_tok) toks[(s0 + i) * max_tok + n] = t;
        bool stop = false;
        if (i == 0) {
#pragma unroll
            for (int q = 0; q < GS_WORDS - GS_STOP0; ++q) stop |= (q < w[GS_NSTOP] && w[GS_STOP0 + q] == t);
        }
        int wt = -1, wr = -1, reset = w[GS_RESET];
        if (!stop && w[GS_UPDATE_PEN]) {                           // gpt_pick_finish's penalty write and reset
            wt = t;
            const int r = reset;
            int tr = 0;
            if (r == n) tr = t;
            else if (r >= 0 && r < n && r < max_tok) {             // token r of this hypothesis' own history
                const int a = min(max(anc_old[(size_t)p * max_tok + r], 0), B - 1);
                tr = min(max(toks[(s0 + a) * max_tok + r], 0), codes - 1);
            }
            if (n + 1 > w[GS_RANGE] && r < max_tok && tr != t) { wr = tr; reset = r + 1; }
        }
        pw_t[i] = wt; pw_r[i] = wr; new_reset[i] = reset;
        if (i == 0) s_done = stop || (w[GS_LIMIT] > 0 && n + 1 >= w[GS_LIMIT]);
    }
    __syncthreads();
    const int gen = sw[0][GS_GEN_LEN] + 1;
    if (tid < B) {
        const int i = tid, p = min(max(sh.parent[i], 0), B - 1);
        int w[GS_WORDS];
#pragma unroll
        for (int q = 0; q < GS_WORDS; ++q) w[q] = sw[p][q];
        w[GS_TOKEN] = min(max(sh.code[i], 0), codes - 1);
        w[GS_NDEC] = n + 1;
        w[GS_RESET] = new_reset[i];
        w[GS_HIST] += rows;
        w[GS_GEN_LEN] = gen;
        w[GS_DONE] = s_done;
        int* so = st + (s0 + i) * GS_WORDS;
#pragma unroll
        for (int q = 0; q < GS_STOP0; q += 4) *reinterpret_cast<int4*>(so + q) = make_int4(w[q], w[q + 1], w[q + 2], w[q + 3]);
        if (GS_STOP0 % 4) { for (int q = GS_STOP0 / 4 * 4; q < GS_STOP0; ++q) so[q] = w[q]; }
        scores[s0 + i] = sh.score[i];
        if (n >= 0 && n < max_tok) anc_new[(size_t)i * max_tok + n] = i;
    }
    const int nprev = min(max(n, 0), max_tok);
    const int g = min(max(gen, 0), max_pos - 1);
    for (int i = 0; i < B; ++i) {
        const int p = min(max(sh.parent[i], 0), B - 1), t = min(max(sh.code[i], 0), codes - 1);
        const int wt = pw_t[i], wr = pw_r[i];
        for (int c = tid; c < codes; c += 1024) {
            float v = pen_old[(size_t)p * codes + c];
            v = c == wt ? repv : v;
            v = c == wr ? 1.f : v;
            pen_new[(size_t)i * codes + c] = v;
        }
        for (int q = tid; q < nprev; q += 1024) anc_new[(size_t)i * max_tok + q] = anc_old[(size_t)p * max_tok + q];
        for (int c = tid; c < hidden; c += 1024) {
            // last_hidden_state row n of this hypothesis: the row of the parent's forward pass
            if (n >= 0 && n < max_tok) hid[((s0 + i) * max_tok + n) * hidden + c] = last[(s0 + p) * hidden + c];
            // graph C for the next decode step (IndexTTS_C.forward, Export_IndexTTS.py:222-225)
            xb[(s0 + i) * hidden + c] = emb[(size_t)t * hidden + c] + pos[(size_t)g * hidden + c];
        }
    }
}

// The decode step's selection: group = group0 + blockIdx.x, slots group * B .. + B - 1.
__global__ __launch_bounds__(1024) void gpt_beam_step_kernel(const float* __restrict__ logits, float* pen0, float* pen1,
                                                             const float* __restrict__ last, int* st, int* toks,
                                                             float* __restrict__ hid, int* anc0, int* anc1, float* scores,
                                                             int codes, int hidden, int rows, const float* __restrict__ rep_dev,
                                                             int max_tok, const float* __restrict__ emb,
                                                             const float* __restrict__ pos, int max_pos, float* __restrict__ xb,
                                                             int B, int first, int group0) {
    beam_step_body(logits, pen0, pen1, last, st, toks, hid, anc0, anc1, scores, codes, hidden, rows, rep_dev, max_tok, emb, pos,
                   max_pos, xb, B, first, (size_t)(group0 + blockIdx.x) * B);
}

// Selection 0 of every group a packed prompt pass admitted, in one launch: workgroup q serves segment q of the pass's table
// (Gpt::Seg as an int4: first packed row, rows, slot, pad), the one the pass's KV scatter and attention read.  The group is
// slot / B — the groups of a pass need not be neighbours — and `rows` is the segment's.  A segment whose slot does not name a
// whole group inside the handle's slots is left alone (block-uniform).
__global__ __launch_bounds__(1024) void gpt_beam_first_segs_kernel(const int4* __restrict__ segs, const float* __restrict__ logits,
                                                                   float* pen0, float* pen1, const float* __restrict__ last,
                                                                   int* st, int* toks, float* __restrict__ hid, int* anc0,
                                                                   int* anc1, float* scores, int codes, int hidden,
                                                                   const float* __restrict__ rep_dev, int max_tok,
                                                                   const float* __restrict__ emb, const float* __restrict__ pos,
                                                                   int max_pos, float* __restrict__ xb, int B, int max_batch) {
    const int4 g = segs[blockIdx.x];
    const int group = g.z / B;
    if (g.z < 0 || (group + 1) * B > max_batch) return;
    beam_step_body(logits, pen0, pen1, last, st, toks, hid, anc0, anc1, scores, codes, hidden, min(max(g.y, 0), max_tok), rep_dev,
                   max_tok, emb, pos, max_pos, xb, B, 1, (size_t)group * B);
}

// Decode-step attention of a hypothesis: gpt_attn1_body (gpt_attn.h) with the slot of every key / value row read from the
// ancestor table.  blockIdx.y = slot; its group's first slot holds the prompt's rows.  A lane's key j >= P sits in slot
// anc[j - P] of the group; the value rows of a pass take their slots from the lanes that hold the same keys.
template <typename T>
__global__ __launch_bounds__(256) void gpt_attn1_beam_kernel(const T* __restrict__ qkv, const T* __restrict__ kc,
                                                             const T* __restrict__ vc, T* __restrict__ out,
                                                             const int* __restrict__ st, const int* __restrict__ anc0,
                                                             const int* __restrict__ anc1, int hidden, int max_seq,
                                                             size_t slot_stride, int B) {
    const int head = blockIdx.x, slot = blockIdx.y;
    const int s0 = slot / B * B;               // the group's first slot
    st += slot * GS_WORDS;
    const int hist = st[GS_HIST], ndec = st[GS_NDEC];
    const int kv = min(max(hist, 0) + 1, max_seq);
    const int P = hist - ndec + 1;             // the prompt's rows: history = P + (selections so far - 1)
    const int* anc = ((ndec & 1) ? anc1 : anc0) + (size_t)slot * max_seq;
    gpt_attn1_body<T>(qkv, kc + (size_t)s0 * slot_stride, vc + (size_t)s0 * slot_stride, out, slot, head, hidden, max_seq, kv,
                      AttnRowsAncestor{anc, P, B, max_seq, slot_stride});
}

void launch_gpt_attn1_beam(int dtype, const void* qkv, const void* kc, const void* vc, void* out, const int* st, const int* anc0,
                           const int* anc1, int heads, int nr, int hidden, int max_seq, size_t slot_stride, int B, hipStream_t s) {
#define ATT(T, ...) hipLaunchKernelGGL(gpt_attn1_beam_kernel<T>, dim3(heads, nr), dim3(256), 0, s, (const T*)qkv, (const T*)kc, (const T*)vc, (T*)out, st, anc0, anc1, hidden, max_seq, slot_stride, B)
    GPT_DISPATCH(ATT, 0);
#undef ATT
}

// hypothesis 0 of every group along its ancestors: token n and last_hidden_state row n were stored by slot anc[n]
__global__ __launch_bounds__(256) void gpt_beam_gather_kernel(const int* __restrict__ st, const int* __restrict__ anc0,
                                                              const int* __restrict__ anc1, const int* __restrict__ toks,
                                                              const float* __restrict__ hid, int32_t* __restrict__ tokens,
                                                              float* __restrict__ hidden_out, int B, int max_tok, int hidden,
                                                              int cap) {
    const size_t s0 = (size_t)blockIdx.y * B;
    const int n = blockIdx.x;
    const int ndec = st[s0 * GS_WORDS + GS_NDEC];
    if (n >= ndec || n >= cap || n >= max_tok) return;
    const int* anc = ((ndec & 1) ? anc1 : anc0) + s0 * max_tok;
    const size_t src = s0 + min(max(anc[n], 0), B - 1);
    if (tokens && threadIdx.x == 0) tokens[(size_t)blockIdx.y * cap + n] = toks[src * max_tok + n];
    if (hidden_out)
        for (int c = threadIdx.x; c < hidden; c += 256)
            hidden_out[((size_t)blockIdx.y * cap + n) * hidden + c] = hid[(src * max_tok + n) * hidden + c];
}

// Retirement of the queue's groups by table, in the style of gpt_copy_out_kernel and of the gather above: entry q = (slot = the
// group's first slot, sentence, count, dst_row).  Token n and last_hidden_state row n of hypothesis 0 were stored by slot anc[n]
// of the group, on the side GS_NDEC & 1 of the state the group still holds; they go to row dst_row + n of the destination arrays
// and hypothesis 0's score to score_dst[sentence] (the caller's (n, cap) arrays and (n) scores, or packed staging buffers).  One
// block per (row of the longest entry, entry); the table travels as a kernel argument.
__global__ __launch_bounds__(256) void gpt_beam_out_kernel(Gpt::OutTable tab, const int* __restrict__ st,
                                                           const int* __restrict__ anc0, const int* __restrict__ anc1,
                                                           const int* __restrict__ toks, const float* __restrict__ hid,
                                                           const float* __restrict__ score, int32_t* __restrict__ tokens_dst,
                                                           float* __restrict__ hidden_dst, float* __restrict__ score_dst, int B,
                                                           int max_tok, int hidden, int max_batch) {
    const Gpt::OutSeg g = tab.e[blockIdx.y];
    const int n = blockIdx.x;
    if (g.slot < 0 || g.slot % B != 0 || g.slot + B > max_batch || g.sentence < 0) return;      // block-uniform
    const size_t s0 = (size_t)g.slot;
    if (n == 0 && threadIdx.x == 0 && score_dst) score_dst[g.sentence] = score[s0];
    const int ndec = st[s0 * GS_WORDS + GS_NDEC];
    if (n >= g.count || n >= ndec || n >= max_tok) return;
    const int* anc = ((ndec & 1) ? anc1 : anc0) + s0 * max_tok;
    const size_t src = s0 + min(max(anc[n], 0), B - 1);
    const size_t dst = (size_t)(g.dst_row + n);
    if (tokens_dst && threadIdx.x == 0) tokens_dst[dst] = toks[src * max_tok + n];
    if (hidden_dst)
        for (int c = threadIdx.x; c < hidden; c += 256) hidden_dst[dst * hidden + c] = hid[(src * max_tok + n) * hidden + c];
}

// ---------------------------------------------------------------------------------------------------------------
// engine
// ---------------------------------------------------------------------------------------------------------------
void launch_gpt_beam_select_rows(const float* logits, const float* pen, const float* prev, int groups, int B, int codes,
                                 int first, int32_t* parents, int32_t* tokens, float* scores, hipStream_t s) {
    MI_REQUIRE(codes >= 1 && codes <= GPT_BEAM_MAX_CODES, "gpt beam: the unit entry supports 1..16384 codes");
    MI_REQUIRE(B >= 1 && B <= GPT_BEAM_MAX && B <= codes, "gpt beam: num_beams must be in [1, 8] and at most the code count");
    MI_REQUIRE(groups >= 1 && logits && (first || prev) && parents && tokens && scores, "gpt beam: selection launch");
    hipLaunchKernelGGL(gpt_beam_select_rows_kernel, dim3(groups), dim3(1024), 0, s, logits, pen, prev, B, codes, first ? 1 : 0,
                       parents, tokens, scores);
    MI_HIP(hipGetLastError());
}

void Gpt::beam_ensure() {
    if (pen_b.p) return;
    const size_t P = MBp;
    pen_b.ensure(P * cfg.mel_codes * 4);
    anc.ensure(2 * P * cfg.max_seq * 4);
    score.ensure(P * 4);
    for (DevBuf* b : {&pen_b, &anc, &score}) MI_HIP(hipMemsetAsync(b->p, 0, b->bytes, stream));
}

static void beam_step_launch(Gpt& e, int groups, int group0, int B, int rows, int first) {
    const GptCfg& c = e.cfg;
    MI_REQUIRE(B >= 1 && B <= GPT_BEAM_MAX && B <= c.mel_codes && group0 >= 0 && groups >= 1 &&
               (group0 + groups) * B <= c.max_batch && e.pen_b.p, "gpt beam: selection launch");
    int* anc0 = e.anc.as<int>();
    hipLaunchKernelGGL(gpt_beam_step_kernel, dim3(groups), dim3(1024), 0, e.stream, e.logits.as<float>(), e.pen.as<float>(),
                       e.pen_b.as<float>(), e.last.as<float>(), e.state.as<int>(), e.toks.as<int>(), e.hid.as<float>(), anc0,
                       anc0 + (size_t)e.MBp * c.max_seq, e.score.as<float>(), c.mel_codes, c.hidden, rows,
                       e.rep_dev.as<float>(), c.max_seq, e.mel_emb.as<float>(), e.mel_pos.as<float>(), c.max_mel_pos,
                       e.Xd.as<float>(), B, first, group0);
    MI_HIP(hipGetLastError());
}

void Gpt::beam_select_first(int group, int B, int rows) { beam_step_launch(*this, 1, group, B, rows, 1); }

// the batched decode step over the nb * B hypotheses, with the attention that follows the ancestor table and the selection
void Gpt::decode_beam_eager(int nb, int B) {
    const int nr = nb * B;
    MI_REQUIRE(nb >= 1 && B >= 1 && nr <= cfg.max_batch && pen_b.p, "gpt beam: batch exceeds max_batch");
    const int* anc0 = anc.as<int>();
    const int* anc1 = anc0 + (size_t)MBp * cfg.max_seq;
    decode_rows_eager(nr, [&](char* kcl, char* vcl) {
        launch_gpt_attn1_beam(dtype, qkvd.p, kcl, vcl, attd.p, state.as<int>(), anc0, anc1, cfg.heads, nr, cfg.hidden, cfg.max_seq,
                              slot_cache_elems(), B, stream);
    }, [&] { beam_step_launch(*this, nb, 0, B, 1, 0); });
}

void Gpt::decode_beam_steps(int nb, int B, int n) {
    check_graph_epoch();
    replay(batch_graphs[{nb * B, 1 + B}], n, [&] { decode_beam_eager(nb, B); });
}

void Gpt::beam_gather(int nb, int B, int32_t* tokens, float* hidden, int cap) {
    MI_REQUIRE(nb >= 1 && B >= 1 && nb * B <= cfg.max_batch && cap >= 1 && pen_b.p, "gpt beam: gather");
    const int* anc0 = anc.as<int>();
    const int rows = cap < cfg.max_seq ? cap : cfg.max_seq;
    hipLaunchKernelGGL(gpt_beam_gather_kernel, dim3(rows, nb), dim3(256), 0, stream, state.as<int>(), anc0,
                       anc0 + (size_t)MBp * cfg.max_seq, toks.as<int>(), hid.as<float>(), tokens, hidden, B, cfg.max_seq,
                       cfg.hidden, cap);
    MI_HIP(hipGetLastError());
}

// selection 0 of the k groups whose segments forward_packed left in segtab, one launch
void Gpt::beam_select_segs(int k, int B) {
    const GptCfg& c = cfg;
    MI_REQUIRE(B >= 1 && B <= GPT_BEAM_MAX && B <= c.mel_codes && k >= 1 && k * B <= c.max_batch && pen_b.p && segtab.p,
               "gpt beam: selection launch over a pass's segments");
    int* anc0 = anc.as<int>();
    hipLaunchKernelGGL(gpt_beam_first_segs_kernel, dim3(k), dim3(1024), 0, stream, segtab.as<int4>(), logits.as<float>(),
                       pen.as<float>(), pen_b.as<float>(), last.as<float>(), state.as<int>(), toks.as<int>(), hid.as<float>(), anc0,
                       anc0 + (size_t)MBp * c.max_seq, score.as<float>(), c.mel_codes, c.hidden, rep_dev.as<float>(), c.max_seq,
                       mel_emb.as<float>(), mel_pos.as<float>(), c.max_mel_pos, Xd.as<float>(), B, c.max_batch);
    MI_HIP(hipGetLastError());
}

void Gpt::beam_out_rows(const OutTable& tab, int n, int B, int32_t* tokens_dst, float* hidden_dst, float* score_dst) {
    MI_REQUIRE(n >= 0 && n <= GPT_MAX_BATCH && B >= 1 && B <= GPT_BEAM_MAX && pen_b.p, "gpt beam: retirement table");
    int rows = 1;                                                 // the score leaves in row 0's block
    for (int q = 0; q < n; ++q) {
        const OutSeg& g = tab.e[q];
        MI_REQUIRE(g.slot >= 0 && g.slot % B == 0 && g.slot + B <= cfg.max_batch && g.count >= 0 && g.count <= cfg.max_seq &&
                       g.sentence >= 0 && g.dst_row >= 0, "gpt beam: retirement entry");
        rows = std::max(rows, (int)g.count);
    }
    if (n == 0 || (!tokens_dst && !hidden_dst && !score_dst)) return;
    const int* anc0 = anc.as<int>();
    hipLaunchKernelGGL(gpt_beam_out_kernel, dim3(rows, n), dim3(256), 0, stream, tab, state.as<int>(), anc0,
                       anc0 + (size_t)MBp * cfg.max_seq, toks.as<int>(), hid.as<float>(), score.as<float>(), tokens_dst, hidden_dst,
                       score_dst, B, cfg.max_seq, cfg.hidden, cfg.max_batch);
    MI_HIP(hipGetLastError());
}

}  // namespace mi
