// gpt.h — IndexTTS acoustic GPT-2 decoder (graphs B, C, E of IndexTTS/Export_IndexTTS.py:203-289) with the KV cache,
// the repeat-penalty vector and the greedy decode loop (Inference_IndexTTS_ONNX.py:745-783) resident on the device.
#pragma once
#include "common.h"
#include "f5_kernels.h"

namespace mi {

struct GptCfg {
    int hidden, layers, heads, inner, mel_codes, text_tokens, max_mel_pos, max_text_pos, max_seq;
    int max_batch = 1;          // sentences decoded together (slots, 1..GPT_MAX_BATCH); optional 10th cfg int
    int head_dim() const { return hidden / heads; }
};
constexpr int GPT_MAX_BATCH = 64;                // slots of one handle: four 16-column MFMA tiles in the decode linears
GptCfg parse_gpt_cfg(const int32_t* ci, int ni);
int64_t gpt_param_count(const GptCfg& c);

// device-side decode state (one int32 array; kernels read it so that a decode step has no host-dependent argument
// and can be captured once into a hipGraph)
enum { GS_HIST = 0, GS_TOKEN = 1, GS_GEN_LEN = 2, GS_NDEC = 3, GS_RESET = 4, GS_DONE = 5, GS_NSTOP = 6, GS_RANGE = 7,
       GS_UPDATE_PEN = 8, GS_LIMIT = 9, GS_STOP0 = 10, GS_WORDS = 16 };

// rows of the batched decode scratch for mb slots: a batched-GEMV template width (2, 4, 8, 16) or a multiple of 16 (above).
// Never 1: gemv_b_kernel stages whole template widths of x rows, and its narrowest width is 2
inline int gpt_padded_rows(int mb) { return mb <= 2 ? 2 : mb <= 4 ? 4 : mb <= 8 ? 8 : (mb + 15) / 16 * 16; }

// a decode-step linear layer as its launchers see it: weights (n, k), fp32 bias (n) or null, both on the device.  wfmt says what w
// holds: GPT_W_DTYPE = elements of `dtype`; GPT_W_Q8 = uint8 rows with one fp32 scale and one uint8 zero point per row
// (w ~ float(q - zp) * scale, gpt_q8.hip), `dtype` then being the activation type alone
enum { GPT_W_DTYPE = 0, GPT_W_Q8 = 1 };
struct GptLin { int dtype; const void* w; const float* bias; int n, k; int wfmt = GPT_W_DTYPE; const float* scale = nullptr; const uint8_t* zp = nullptr; };

struct GptSampleRec;      // gpt_pick.h
struct GptPoolCfg;        // gpt_pool.h
struct GptPoolDev;

struct Gpt {
    GptCfg cfg;
    int dtype, device;
    hipStream_t stream = nullptr;

    int wfmt = GPT_W_DTYPE;   // what the six matrix kinds (c_attn, attn.c_proj, c_fc, mlp.c_proj, lm_head.1) are stored as
    struct GLin { DevBuf w, b, sc, zp; int n = 0, k = 0; };      // sc / zp: GPT_W_Q8 only
    GptLin lin(const GLin& l) const { return {dtype, l.w.p, l.b.as<float>(), l.n, l.k, wfmt, l.sc.as<float>(), l.zp.as<uint8_t>()}; }
    DevBuf wdq;               // GPT_W_Q8: the 16-bit copy of the matrix a prompt pass is about to use (the largest of the six)
    int64_t weight_bytes() const;                      // device bytes held for the six matrix kinds (mi_gpt_weight_bytes)
    struct Layer { DevBuf ln1_w, ln1_b, ln2_w, ln2_b; GLin qkv, proj, fc, fc2; };
    std::vector<Layer> L;
    DevBuf text_emb, text_pos, mel_emb, mel_pos;       // fp32 tables
    DevBuf lnf_w, lnf_b, fn_w, fn_b;
    GLin head;

    DevBuf kc, vc;            // [slot][layer][head][max_seq][D] in the engine dtype
    DevBuf X, xn, qkv, att, ff;                       // prompt-pass scratch (max_seq rows), shared by the slots
    DevBuf logits, last, pen, toks, hid, state;       // per slot: [slot][codes] / [slot][h] / [slot][max_seq](x h) / words
    DevBuf Xd, xnd, qkvd, attd, ffd, zd;              // batched decode step: one row per slot
    int MBp = 2;              // gpt_padded_rows(max_batch)
    // decode step over nb slots, keyed by (nb, sampled); beam steps: (nb * beams, 1 + beams), in pool mode (nb * beams, 9 + beams)
    std::map<std::pair<int, int>, hipGraphExec_t> batch_graphs;
    DevBuf io_a, io_b, io_s;  // host<->device staging (io_s: scores of a queue round)
    DevBuf rep_dev;           // REPEAT_PENALITY as a device scalar (read by gpt_pick_kernel, also inside replayed graphs)
    void set_rep_value(float v);
    int history = 0;          // host mirror of state[GS_HIST] (valid outside generate())

    // token choice of the calls that follow: 0 = greedy (gpt_pick_kernel), 1 = sampled (gpt_sample_kernel reading `samp`).
    // The C-ABI entry sets it; every launch site and every captured graph is per mode.
    int sampled = 0;
    DevBuf samp;              // per slot: GptSampleRec (gpt_pick.h), beside the GS_* state and not part of it
    void set_sampling(const void* recs, int nb);      // host GptSampleRec[nb] -> samp (synchronous)
    void set_sampling_slot(const void* rec, int slot);   // one slot's record; the other slots' records stay (synchronous)
    void reset_penalty(int slot);                     // one slot's penalty row := ones, in stream order (gpt_prompt.hip)
    // beam search (gpt_beam.hip; the definition is in include/mi355tts.h): a sentence's hypotheses sit in `beams` consecutive
    // slots.  What follows a hypothesis from slot to slot exists twice, the side in use being GS_NDEC & 1: the penalty vectors
    // (side 0 = pen, side 1 = pen_b) and the ancestor table anc[side][slot][n] = the slot inside the group that held this
    // hypothesis' ancestor after selection n — the cache row, token and last_hidden_state row of step n are read from there.
    int beams = 0;            // 0 outside the beam entries; forward_rows / forward_packed then leave the token choice to selection 0
    DevBuf pen_b, anc, score; // allocated by the first beam call
    void beam_ensure();
    void beam_select_first(int group, int B, int rows);                               // selection 0 after a prompt pass
    void decode_beam_eager(int nb, int B);                                            // one step of nb * B hypotheses + selection
    void decode_beam_steps(int nb, int B, int n);
    // hypothesis 0 of every group, gathered along its ancestors: tokens (nb, cap), hidden (nb, cap, hidden), device arrays
    void beam_gather(int nb, int B, int32_t* tokens, float* hidden, int cap);
    // the sentence queue with beams: selection 0 of the k groups of the packed pass just run (their segments are in segtab), in
    // one launch; retirement of the table's groups along their ancestor tables, with hypothesis 0's scores, in one launch
    void beam_select_segs(int k, int B);
    // beam search with a finished pool (gpt_beam_pool.hip): the decode step and attention above with a selection kernel of its
    // own; the pool of every group, its frozen ancestor lists and last rows, the key scratch and the call's parameters
    DevBuf pool_score, pool_meta, pool_anc, pool_hid, pool_keys, pool_cfg, pool_rec;      // allocated by the first pool call
    void pool_ensure();
    GptPoolDev pool_dev();
    void pool_begin(int nb, int B, const GptPoolCfg& cf, const GptSampleRec* recs);      // empty pools; recs: nb records or null
    void pool_select_first(int group, int B, int rows);
    void decode_pool_eager(int nb, int B);
    void decode_pool_steps(int nb, int B, int n);
    void pool_gather(int nb, int B, int32_t* tokens, float* hidden, int cap);          // pool entry 0 of every group
    // the sentence queue in pool mode: `pool` set beside `beams` makes forward_packed run the pool-mode selection 0; the
    // session's parameters; one group's pool made empty in stream order (rec: the sentence's record, null = deterministic);
    // selection 0 of the k groups of the pass just run, one launch; retirement of the table's groups along their frozen
    // lists (pool entry 0's tokens, rows and score), one launch
    int pool = 0;
    void pool_set_cfg(const GptPoolCfg& cf);
    void pool_reset_group(int group, int B, const GptSampleRec* rec);
    void pool_select_segs(int k, int B);              // (pool_out_rows: below, beside beam_out_rows)
    hipGraphExec_t step_graph[2] = {nullptr, nullptr};      // by mode
    bool use_graph = true;
    long graph_epoch = 0;     // option_epoch() the captured graphs were taken under
    void check_graph_epoch();
    // n decode steps: `step` launches one.  With graphs on, the first step ever taken under this key runs eagerly (one-time
    // lazy initialisation stays out of the capture), the second is captured into `exec`, the rest are replays; an
    // instantiation failure turns graphs off for the handle and the steps run eagerly.
    template <typename F> void replay(hipGraphExec_t& exec, int n, F&& step);

    Gpt(const GptCfg& c, const float* w, int64_t nw, int dt, int dev, int wfmt = GPT_W_DTYPE);
    ~Gpt();

    void text_embed(const int32_t* ids_dev, int n, float* out_dev);                 // graph B (n + 2 rows)
    void mel_embed(int32_t id, long gen_len, float* out_dev);                        // graph C
    void reset();
    // graph E on rows new positions whose hidden states are already in X[0..rows): fills last / logits / state token
    void forward_rows(int rows, int flag, int slot = 0);
    // the token of a prompt pass or single step from the slot's logits / last row (greedy or sampled by `sampled`) and the
    // driver loop's bookkeeping; x0: slot 0 also gets graph C of that token in X row 0 (the single-sentence decode step's input)
    void choose_token(int rows, int slot, bool x0);
    // packed prompt pass (gpt_prompt.hip): k prompts lie back to back in X, segment g = rows [first, first + rows) -> slot,
    // ascending `first`, no gaps, the total within max_seq, every slot's history 0 and at most once.  One pass over the weights
    // for all of them, then per segment what the tail of forward_rows does on its last row.
    struct Seg { int32_t first, rows, slot, pad; };
    DevBuf segtab;            // the pass's segments on the device (max_batch entries)
    bool packed_ready = false;
    void forward_packed(const Seg* segs, int k);
    // queue sessions (gpt_queue.hip): tokens and last_hidden_state rows [first, first + count) of `slot` -> rows dst_row .. of the
    // destination arrays (either may be null), every entry of the table in ONE launch, in stream order (gpt_prompt.hip)
    struct OutSeg { int32_t slot, first, count, sentence; int64_t dst_row; };
    struct OutTable { OutSeg e[GPT_MAX_BATCH]; };
    void copy_out_rows(const OutTable& tab, int n, int32_t* tokens_dst, float* hidden_dst);
    void beam_out_rows(const OutTable& tab, int n, int B, int32_t* tokens_dst, float* hidden_dst, float* score_dst);   // gpt_beam.hip
    void pool_out_rows(const OutTable& tab, int n, int B, int32_t* tokens_dst, float* hidden_dst, float* score_dst);   // gpt_beam_pool.hip
    // one layer's K / V cache of a slot (bytes; slots are slot_cache_elems() elements apart)
    struct LayerKV { char *k, *v; };
    LayerKV layer_cache(int layer, int slot = 0) {
        const size_t off = ((size_t)slot * slot_cache_elems() + (size_t)layer * cfg.hidden * cfg.max_seq) * dtype_size(dtype);
        return {(char*)kc.p + off, (char*)vc.p + off};
    }
    void set_state(const std::vector<int32_t>& words, int slot = 0);
    std::vector<int32_t> get_state(int slot = 0);
    // the greedy or sampled token choice (by `sampled`) of slots slot0 .. slot0 + nb - 1 from their logits / last rows, with
    // the driver loop's bookkeeping and graph C of the token in the slot's batched decode row; xa: a second copy of slot0's
    void launch_choice(int nb, int slot0, int rows, float* xa);
    // one batched decode step over rows 0 .. nr-1 of the decode scratch: the layer loop with `attn(kcl, vcl)` as the
    // attention launch of a layer (slot 0's cache of that layer), then ln_f / final_norm / lm_head, then `tail()`
    template <typename A, typename F> void decode_rows_eager(int nr, A&& attn, F&& tail);
    void decode_batch_eager(int nb);                                                 // one token for slots 0..nb-1
    void decode_batch_steps(int nb, int n);
    // tuning: microseconds per launch of the token-choosing kernel of the current mode over nb slots, on the logits the last step
    // left (every slot is marked done for the measurement, so nothing but the choice runs and no state moves)
    double bench_pick(int nb, int iters);
    void gemv_b(const GLin& l, const void* x, int nb, void* out, int odt, int act, const float* res, void* kcl, void* vcl);
    // gemv_b for nb <= 16 rows whose state words start at st (a 16-slot group of a wider batch passes its own bases)
    void gemv_b16(const GLin& l, const void* x, int nb, void* out, int of, int act, const float* res, void* kcl, void* vcl,
                  const int* st);
    size_t slot_cache_elems() const { return (size_t)cfg.layers * cfg.hidden * cfg.max_seq; }
    void decode_step_eager();                                                        // C (from state) + E + bookkeeping
    void decode_steps(int n);                                                        // n graph replays
    void kv_read(int layer, float* keys_dev, float* values_dev);                      // slot 0
    void kv_write(int layer, const float* keys_dev, const float* values_dev, int hist);
    void linear(const GLin& l, const void* x, int rows, void* out, int odt, int act, const float* res);
    void gemv(const GLin& l, const void* x, const float* ln_w, const float* ln_b, void* out, int odt, int act,
              const float* res, void* kcl, void* vcl, int slot = 0, const float* pre_w = nullptr, const float* pre_b = nullptr,
              float* pre_out = nullptr);
};

// KERNEL(T, ...) for the engine's dtype (a member `dtype` is in scope), then the launch check
#define GPT_DISPATCH(KERNEL, ...)                                                     \
    do {                                                                              \
        if (dtype == MI_F32) { KERNEL(float, __VA_ARGS__); }                          \
        else if (dtype == MI_F16) { KERNEL(f16, __VA_ARGS__); }                       \
        else { KERNEL(bf16, __VA_ARGS__); }                                           \
        MI_HIP(hipGetLastError());                                                    \
    } while (0)

template <typename A, typename F> void Gpt::decode_rows_eager(int nr, A&& attn, F&& tail) {
    const int h = cfg.hidden;
    hipStream_t s = stream;
    float* x = Xd.as<float>();                 // row b = graph C of slot b's state, written by the choice or selection before
    for (int li = 0; li < cfg.layers; ++li) {
        Layer& l = L[li];
        const LayerKV kv = layer_cache(li);
        launch_rownorm(NORM_LN_AFFINE, x, xnd.p, dtype, l.ln1_w.as<float>(), l.ln1_b.as<float>(), nr, h, 1e-5f, s);
        gemv_b(l.qkv, xnd.p, nr, qkvd.p, dtype, ACT_NONE, nullptr, kv.k, kv.v);
        {
            ProfScope ps(FAM_ATTN, s, 0.0, 0.0);
            attn(kv.k, kv.v);
        }
        gemv_b(l.proj, attd.p, nr, x, MI_F32, ACT_NONE, x, nullptr, nullptr);
        launch_rownorm(NORM_LN_AFFINE, x, xnd.p, dtype, l.ln2_w.as<float>(), l.ln2_b.as<float>(), nr, h, 1e-5f, s);
        gemv_b(l.fc, xnd.p, nr, ffd.p, dtype, ACT_GELU_TANH, nullptr, nullptr, nullptr);
        gemv_b(l.fc2, ffd.p, nr, x, MI_F32, ACT_NONE, x, nullptr, nullptr);
    }
    launch_rownorm(NORM_LN_AFFINE, x, last.p, MI_F32, lnf_w.as<float>(), lnf_b.as<float>(), nr, h, 1e-5f, s);
    launch_rownorm(NORM_LN_AFFINE, last.as<float>(), zd.p, dtype, fn_w.as<float>(), fn_b.as<float>(), nr, h, 1e-5f, s);
    gemv_b(head, zd.p, nr, logits.p, MI_F32, ACT_NONE, nullptr, nullptr, nullptr);
    tail();
}

template <typename F> void Gpt::replay(hipGraphExec_t& exec, int n, F&& step) {
    if (n <= 0) return;
    if (!use_graph || prof_mask() != 0) { for (int i = 0; i < n; ++i) step(); return; }
    if (!exec) {
        step();
        --n;
        hipGraph_t graph = nullptr;
        MI_HIP(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
        try {
            step();
        } catch (...) {
            (void)hipStreamEndCapture(stream, &graph);
            if (graph) (void)hipGraphDestroy(graph);
            throw;
        }
        MI_HIP(hipStreamEndCapture(stream, &graph));
        hipError_t err = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (err != hipSuccess) { exec = nullptr; use_graph = false; for (int i = 0; i < n; ++i) step(); return; }
    }
    for (int i = 0; i < n; ++i) MI_HIP(hipGraphLaunch(exec, stream));
}

// The decode-step linear launches (gpt.hip), called by Gpt::gemv / gemv_b / gemv_b16 and by the unit entries of capi.hip
// (mi_gpt_linear_*): x, out, res, kcl / vcl (one layer's cache of the first slot, null = no QKV epilogue) on the device, st = the
// GS_* state words of the first row's slot.  odt = MI_F32 or the layer's dtype.
//   one row (gemv_d_kernel): x of l.dtype, or the fp32 residual row when ln_w / ln_b are given (LayerNorm fused in; pre_w / pre_b:
//   a LayerNorm in front of that one, its fp32 row also stored to pre_out)
void launch_gpt_gemv(const GptLin& l, const void* x, const float* ln_w, const float* ln_b, const float* pre_w, const float* pre_b,
                     float* pre_out, void* out, int odt, int act, const float* res, void* kcl, void* vcl, const int* st,
                     int max_seq, hipStream_t s);
//   nb rows, row b = slot b (state words st + b * GS_WORDS, cache slot_stride elements on).  The kernels read whole template widths
//   of x rows: x holds max_rows >= nb rows, max_rows as Gpt::MBp
void launch_gpt_gemv_b(const GptLin& l, const void* x, int nb, int max_rows, void* out, int odt, int act, const float* res,
                       void* kcl, void* vcl, const int* st, int max_seq, size_t slot_stride, hipStream_t s);
//   nb <= 16 rows (a 16-slot group of a wider batch passes its own bases); of = the output is fp32
void launch_gpt_gemv_b16(const GptLin& l, const void* x, int nb, void* out, int of, int act, const float* res, void* kcl, void* vcl,
                         const int* st, int max_seq, size_t slot_stride, hipStream_t s);

// The same launches on GPT_W_Q8 layers (gpt_q8.hip; the three above route to them): K a multiple of 16, MI_F16 activations.
// launch_gpt_gemv_wide_q8 is the 17..64-row matrix-core launch and returns false when the options or K rule it out (the caller then
// goes group by group); launch_gpt_dequant_q8 writes the layer's (n, k) matrix as f16(float(q - zp) * scale) to `out`.
void launch_gpt_gemv_q8(const GptLin& l, const void* x, const float* ln_w, const float* ln_b, const float* pre_w, const float* pre_b,
                        float* pre_out, void* out, int odt, int act, const float* res, void* kcl, void* vcl, const int* st,
                        int max_seq, hipStream_t s);
void launch_gpt_gemv_b16_q8(const GptLin& l, const void* x, int nb, void* out, int of, int act, const float* res, void* kcl, void* vcl,
                            const int* st, int max_seq, size_t slot_stride, hipStream_t s);
bool launch_gpt_gemv_wide_q8(const GptLin& l, const void* x, int nb, void* out, int of, int act, const float* res, void* kcl,
                             void* vcl, const int* st, int max_seq, size_t slot_stride, hipStream_t s);
void launch_gpt_dequant_q8(const GptLin& l, void* out, hipStream_t s);
// per-row asymmetric uint8 quantisation of (n, k) fp32 rows on the host (the rule is stated in include/mi355tts.h)
void gpt_quantize_u8(const float* w, int n, int k, uint8_t* q, float* scale, uint8_t* zp);

// The four attention launches of the GPT, each defined beside its kernel and called by the engine and by the unit entries of
// capi.hip (mi_gpt_attn_*): arrays of `dtype` on the device, st = GS_* state words, kc / vc = one layer's cache.
//   decode step (gpt.hip): rows 0 .. nrows-1 of qkv / out.  batched: row r is slot r (its state words, its cache slot_stride
//   elements on); otherwise one row against st / kc / vc as given
void launch_gpt_attn1(int dtype, const void* qkv, const void* kc, const void* vc, void* out, const int* st, int heads, int nrows,
                      int hidden, int max_seq, int batched, size_t slot_stride, hipStream_t s);
//   decode step of nr hypotheses in groups of B slots (gpt_beam.hip): kc / vc = slot 0's layer, anc0 / anc1 = the two sides of
//   the ancestor table, [slot][max_seq] each
void launch_gpt_attn1_beam(int dtype, const void* qkv, const void* kc, const void* vc, void* out, const int* st, const int* anc0,
                           const int* anc1, int heads, int nr, int hidden, int max_seq, size_t slot_stride, int B, hipStream_t s);
//   a lone prompt's `rows` new rows behind st[GS_HIST] cached ones (gpt.hip); dynamic LDS = gpt_prompt_attn_lds(max_seq)
void launch_gpt_attn_prompt(int dtype, const void* qkv, const void* kc, const void* vc, void* out, const int* st, int heads,
                            int rows, int flag, int hidden, int max_seq, hipStream_t s);
//   `total` packed rows over the nseg segments of the device table segs (gpt_prompt.hip): kc / vc = slot 0's layer; dynamic
//   LDS = gpt_packed_attn_lds(max_seq)
void launch_gpt_attn_packed(int dtype, const void* qkv, const void* kc, const void* vc, void* out, const void* segs, int nseg,
                            int total, int heads, int hidden, int max_seq, int max_batch, size_t slot_stride, hipStream_t s);
// dynamic LDS of the two prompt kernels, in bytes.  Above the 64 KiB a launch may ask for by default the caller raises
// hipFuncAttributeMaxDynamicSharedMemorySize first (gpt_attn_prompt_reserve / gpt_attn_packed_reserve, all three types).
inline int gpt_prompt_attn_lds(int max_seq) { return (max_seq + 64 + 512) * 4; }                  // sc | qs | red
inline int gpt_packed_attn_lds(int max_seq) { return (((max_seq + 3) & ~3) + 64 + 512 + 4) * 4; } // sc | qs | red | bc
void gpt_attn_prompt_reserve(int lds);
void gpt_attn_packed_reserve(int lds);

constexpr int GPT_BEAM_MAX = 8;                  // hypotheses per sentence
constexpr int GPT_BEAM_MAX_CODES = 16384;        // the unit entry's documented range
// gpt_beam.hip: one selection per group on rows of logits (mi_gpt_beam_select): device arrays of groups * B rows, pen may be null
void launch_gpt_beam_select_rows(const float* logits, const float* pen, const float* prev, int groups, int B, int codes,
                                 int first, int32_t* parents, int32_t* tokens, float* scores, hipStream_t s);

}  // namespace mi
