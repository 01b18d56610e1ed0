/*
 * mi355tts.h — C-ABI of libmi355tts.so, the MI355X (gfx950) engine that stands in for the
 * reference's onnxruntime.InferenceSession.run() hot path.
 *
 * Each entry point names the reference interface it replaces (paths relative to the
 * reference repo DakeQQ/Text-to-Speech-TTS-ONNX):
 *
 *   mi_bigvgan_forward      ort_session_A.run_with_ort_values([generated_wav], {mel_features})
 *                           BigVGAN/Export_BigVGAN.py:170   (graph = BIGVGAN.forward, :44-49)
 *   mi_f5_preprocess        ort_session_A.run(...)   F5_TTS/F5-TTS-ONNX-Inference.py:247-253
 *                           (graph = F5Preprocess.forward, F5_TTS/Export_F5.py:117-141)
 *   mi_f5_transformer_step  ort_session_B.run(...)   F5_TTS/F5-TTS-ONNX-Inference.py:292-303
 *                           (graph = F5Transformer.forward, F5_TTS/Export_F5.py:167-182)
 *   mi_f5_sample            the whole `for i in range(0, NFE_STEP - 1, FUSE_NFE)` loop, :291-304,
 *                           kept on device (no per-step host round trip)
 *   mi_f5_decode            ort_session_C.run(...)   F5_TTS/F5-TTS-ONNX-Inference.py:306-311
 *                           (graph = F5Decode.forward, F5_TTS/Export_F5.py:193-203)
 *
 * Conventions
 *   - plain pointers + sizes, no C++/torch types; tensors are row-major contiguous with exactly
 *     the ONNX graph layouts.
 *   - `mem` says where caller buffers live: MI_HOST (copied by the engine) or MI_DEVICE (HIP
 *     device pointers on the handle's device, e.g. torch tensor.data_ptr()).
 *   - every function returns 0 on success, a negative MI_E* code on failure; mi_last_error()
 *     gives the message (thread-local).  Constructors return NULL on failure.
 *   - a handle owns its weights, workspace and one HIP stream; calls on one handle are
 *     serialised; different handles may be used concurrently from different threads.
 *   - weights are one flat fp32 blob in the canonical tensor order of
 *     mi355tts/weights.py (bigvgan_spec / f5_packed_spec), PyTorch-native layouts, with the
 *     reference's export-time folds already applied by the packer.
 */
#ifndef MI355TTS_H
#define MI355TTS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { MI_F32 = 0, MI_F16 = 1, MI_BF16 = 2 };          /* activation / matmul-operand dtype   */
enum { MI_HOST = 0, MI_DEVICE = 1 };                    /* where caller buffers live           */
enum { MI_OK = 0, MI_EINVAL = -1, MI_EHIP = -2, MI_ENOMEM = -3, MI_ESTATE = -4 };

typedef struct mi_bigvgan mi_bigvgan;
typedef struct mi_f5 mi_f5;

/* ---- process-level ------------------------------------------------------------------------ */
int         mi_init(int device);            /* hipSetDevice + context warm-up                  */
int         mi_device_count(void);
const char* mi_last_error(void);
const char* mi_version(void);

/* ---- BigVGAN-v2 vocoder ---------------------------------------------------------------------
 * cfg: int32 array = BigVGANConfig.to_int_array():
 *   [num_mels, initial_channel, n_up, n_kernels, bias_at_final, tanh_at_final, snake_logscale,
 *    rates[n_up], up_kernels[n_up], res_kernels[n_kernels], n_dil, dil[n_kernels][n_dil],
 *    pre_layernorm, speaker_cond]   (the last two are optional; 1,1 = IndexTTS graph F)          */
int64_t     mi_bigvgan_param_count(const int32_t* cfg, int n_cfg);
mi_bigvgan* mi_bigvgan_create(const int32_t* cfg, int n_cfg, const float* weights, int64_t n_weights,
                              int dtype, int device);
/* same, with the blob in host (MI_HOST) or device (MI_DEVICE) memory, e.g. the buffer an RCCL broadcast filled (the
 * broadcast itself is torch.distributed's: SURVEY.md 8b `mi_bcast_weights` became "hand the engine the device buffer").
 * BigVGAN / GPT re-lay their conv weights out in host code, so a device blob is read back once at load; F5 converts its
 * matrices device-to-device (see mi_f5_create_mem).                                                                  */
mi_bigvgan* mi_bigvgan_create_mem(const int32_t* cfg, int n_cfg, const float* weights, int64_t n_weights,
                                  int dtype, int device, int mem);
void        mi_bigvgan_destroy(mi_bigvgan* h);
int64_t     mi_bigvgan_out_len(const mi_bigvgan* h, int frames);      /* frames*hop + 30 */
/* mel: (B, num_mels, frames) fp32 channels-first (the ONNX `mel_features` layout; B>1 is this
 * engine's extension).  out: (B, 1, out_len) int16 = trunc(clamp(32767*tanh(.)))               */
int         mi_bigvgan_forward(mi_bigvgan* h, const float* mel, int B, int frames, int16_t* out, int mem);
/* same, but the float waveform before the int16 conversion (tests)                            */
int         mi_bigvgan_forward_f32(mi_bigvgan* h, const float* mel, int B, int frames, float* out, int mem);
/* IndexTTS graph F (speaker-conditioned vocoder): ort_session_F.run_with_ort_values, IndexTTS/Inference_IndexTTS_ONNX.py:787
 * (graph = IndexTTS_F.forward, IndexTTS/Export_IndexTTS.py:300-314).  The handle must be created from a config with the
 * pre_layernorm / speaker_cond flags (BigVGANConfig.indextts()).  latent: `save_hidden_state` (T_codes, gpt_dim) fp32
 * (the last two rows are dropped, like the reference); conds: save_bigvgan_conds_0..n-1 followed by
 * bigvgan_cond_layer_speaker_embedding, concatenated (n_conds floats).  out: int16 (1,1,(T_codes-2)*hop+30).            */
int         mi_bigvgan_forward_latent(mi_bigvgan* h, const float* latent, int T_codes, const float* conds, int64_t n_conds,
                                      int16_t* out, float* out_f32, int mem);
/* Ragged batch: B items of different lengths in one forward.  frames[b] = F_b (host int64); mel = the items' (num_mels, F_b)
 * channels-first arrays concatenated.  out_i16 (and out_f32 when not NULL) receive the waveforms concatenated, out_lens[b] =
 * F_b * hop + 30; data arrays follow `mem`.  The batch runs as padded slabs of Fmax = max F_b frames; every layer stores zeros
 * past an item's live rows, so item b gets the waveform a forward of it alone gives.  MI_EINVAL, with the handle still usable,
 * for B < 1, F_b < 1, Fmax past the uniform path's limit, out_cap below the sum of out_lens, or a graph-F handle.           */
int         mi_bigvgan_forward_ragged(mi_bigvgan* h, int B, const float* mel, const int64_t* frames, int16_t* out_i16,
                                      float* out_f32, int64_t out_cap, int64_t* out_lens, int mem);
/* ... and IndexTTS graph F for B sentences of one speaker: latent = the items' (t_codes[b], gpt_dim) rows concatenated (the last
 * two rows of each are dropped, like mi_bigvgan_forward_latent; t_codes[b] >= 3, host int64); conds = one conditioning vector
 * in the layout of mi_bigvgan_forward_latent.  This is the one-voice form of mi_bigvgan_forward_latent_voices (n_voices = 1,
 * voice_of = 0 ... 0): the same forward, the same kernels.  out_lens[b] = (t_codes[b] - 2) * hop + 30.                      */
int         mi_bigvgan_forward_latent_ragged(mi_bigvgan* h, int B, const float* latent, const int64_t* t_codes, const float* conds,
                                             int64_t n_conds, int16_t* out_i16, float* out_f32, int64_t out_cap, int64_t* out_lens,
                                             int mem);
/* ... and for B sentences of several speakers in one forward: conds = (n_voices, n_conds) fp32, row-major, every row in the layout
 * of mi_bigvgan_forward_latent (follows `mem`); voice_of[b] (host int32, B values in [0, n_voices)) names item b's row.  A kernel
 * builds the (B, n_conds) table of layer bias + conditioning on the device and conv_pre and the upsamplers read their bias by
 * item, so with mem = MI_DEVICE the conditioning never visits the host.  Item b gets the waveform a forward of it alone with
 * voice voice_of[b] gives.  The remaining arguments are those of mi_bigvgan_forward_latent_ragged.  MI_EINVAL, with the handle
 * still usable, for n_voices < 1, a voice_of[b] outside [0, n_voices), n_conds other than the handle's total, a handle that is
 * not graph F, and everything mi_bigvgan_forward_latent_ragged rejects.                                                     */
int         mi_bigvgan_forward_latent_voices(mi_bigvgan* h, int B, const float* latent, const int64_t* t_codes, int n_voices,
                                             const float* conds, int64_t n_conds, const int32_t* voice_of, int16_t* out_i16,
                                             float* out_f32, int64_t out_cap, int64_t* out_lens, int mem);
/* ... and for WINDOWS of latent rows, so that audio can leave before a sentence has all its rows.  latent = any (latent_rows,
 * gpt_dim) fp32 array (follows `mem`; it may be the `hidden` output of a GPT call where it lies in HBM); item b is frames
 * [row0[b], row0[b] + rows[b]) of it (host int64).  Items may overlap and share rows, and NO rows are dropped here: the caller
 * leaves a sentence's last two rows out of its windows.  head[b] / tail[b] (host int32, >= 0, head + tail < rows) count the halo
 * frames at the window's two ends: their samples are computed and discarded.  Run alone, frames [lo, hi) of a sentence give
 * (hi - lo) * hop + 30 samples, and sample j of them stands for sample lo * hop + j of the sentence's waveform.  The samples kept
 * are [head ? head * hop + 15 : 0, tail ? (rows - tail) * hop + 15 : rows * hop + 30), written concatenated; out_lens[b] is
 * their count, and nothing is written outside the sum of them.  A sample is the sentence's own, to the last bit of the arithmetic,
 * when the halo covers the generator's receptive field (BigVGANConfig.halo_frames(): 34 frames for the IndexTTS-1.5 vocoder); a
 * shorter halo is the caller's trade of accuracy for work.  The forward is that of mi_bigvgan_forward_latent_voices (same slabs,
 * same length-aware launches, same bias table), with row0 as the row-offset table and a windowed conv_post; with head = tail = 0
 * and windows naming whole sentences minus their last two rows it gives that entry's waveforms bit for bit.  n_voices, conds,
 * n_conds, voice_of: as there.  MI_EINVAL, with the handle still usable, for B < 1, rows < 1, head or tail < 0, head + tail >=
 * rows, a window outside [0, latent_rows), a window past the ragged path's frame limit, out_cap below the sum of out_lens, a
 * handle that is not graph F, and everything mi_bigvgan_forward_latent_voices rejects.                                      */
int         mi_bigvgan_forward_latent_windows(mi_bigvgan* h, int B, const float* latent, int64_t latent_rows, const int64_t* row0,
                                              const int64_t* rows, const int32_t* head, const int32_t* tail, int n_voices,
                                              const float* conds, int64_t n_conds, const int32_t* voice_of, int16_t* out_i16,
                                              float* out_f32, int64_t out_cap, int64_t* out_lens, int mem);
/* unit-level entry (tests): one anti-aliased SnakeBeta Activation1d on x (B,C,T) fp32
 * channels-first host memory; post!=0 selects the pad-15 variant (out T+30).                   */
int         mi_aa_activation1d(const float* x, int B, int C, int T, const float* alpha_log,
                               const float* beta_log, int logscale, int post, int dtype, float* y);
/* unit-level entry (tests): the FUSED kernel of the low-channel stages — Activation1d(SnakeBeta) -> Conv1d(C, C, k, dilation,
 * "same" padding) (+ res): `xt = c(a(x))` / `x = c2(a2(xt)) + x` of AMPBlock1.forward, BigVGAN/modeling_modified/
 * bigvgan.py:132-140.  x, res, y: (B, C, T) fp32 channels-first host memory; w (C, C, k); C % 8 == 0, C <= 96.             */
int         mi_aa_conv1d(const float* x, int B, int C, int T, const float* alpha_log, const float* beta_log, int logscale,
                         const float* w, const float* bias, int k, int dilation, const float* res, int dtype, float* y);
/* unit-level entry (tests): Conv1d / ConvTranspose1d on fp32 channels-first host tensors,
 * executed by the implicit-GEMM MFMA kernel in `dtype`.                                       */
int         mi_conv1d(const float* x, int B, int Cin, int T, const float* w, const float* bias, int Cout,
                      int k, int dilation, int padding, int groups, int dtype, float* y);
int         mi_conv_transpose1d(const float* x, int B, int Cin, int T, const float* w, const float* bias,
                                int Cout, int k, int stride, int padding, int dtype, float* y);

/* ---- F5-TTS (DiT CFM sampler + text/mel front end + Vocos/ISTFT back end) ---------------------
 * cfg_i = F5Config.to_int_array() (21 ints: dim, depth, heads, dim_head, ff_mult, mel_dim, text_dim,
 *   text_num_embeds, conv_layers, conv_mult, pos_conv_kernel, pos_conv_groups, freq_embed_dim, nfe_step,
 *   max_signal_length, n_fft, hop_length, sample_rate, vocos_dim, vocos_intermediate, vocos_layers);
 * cfg_f = [cfg_strength, sway_coef] or [cfg_strength, sway_coef, attn_score_scale].  The third value (MI_F16 engines
 * only; absent = 1) selects the attention rounding points of the reference's fp16-transformer export
 * (use_fp16_transformer, F5_TTS/Export_F5.py:20,321-326; F5/fp16/modules.py:467): the caller folds head_dim^-0.25 * 0.1
 * into the q / k projections of the blob (mi355tts.weights.fold_f5 does, from F5Config.ref_fp16_attn), the kernel rounds
 * the q k scores to fp16 and multiplies them by attn_score_scale (= 100) in fp32 before the fp32 softmax.  `dtype` selects the DiT operand type (fp32 residual stream and
 * fp32 softmax/norm statistics always); the front end and the vocoder always run in fp32, like the
 * reference's CPU-pinned graphs A and C (F5-TTS-ONNX-Inference.py:173,214).
 * Batching extension: U utterances of equal max_duration N; tensors gain a leading U axis (utterances of
 * different lengths: mi_f5_synthesize_ragged).                                                        */
int64_t     mi_f5_param_count(const int32_t* cfg_i, int n_i, const float* cfg_f, int n_f);
mi_f5*      mi_f5_create(const int32_t* cfg_i, int n_i, const float* cfg_f, int n_f, const float* weights,
                         int64_t n_weights, int dtype, int device);
/* blob in host or device memory.  MI_DEVICE: every DiT / Vocos matrix (98 % of the blob) is converted to the engine
 * dtype by a device kernel straight out of the caller's buffer — no host staging; only the tensors whose load-time tables
 * are built by host code (time MLP, the two k31 grouped convs, the Vocos embed conv: ~6 M of 351 M floats) are read back. */
mi_f5*      mi_f5_create_mem(const int32_t* cfg_i, int n_i, const float* cfg_f, int n_f, const float* weights,
                             int64_t n_weights, int dtype, int device, int mem);
void        mi_f5_destroy(mi_f5* h);
/* load-time tables (tests): time_expand (nfe, dim), delta_t (nfe-1)   Export_F5.py:153-164          */
int         mi_f5_tables(mi_f5* h, float* time_expand, float* delta_t);
/* What the engine is doing, machine-readably (no reference counterpart: ONNX Runtime has one arithmetic).  Keys:
 *   "f32_arithmetic"     fp32 engines: 0 native fp32 MFMA | 2 fp16 {hi, lo} pairs | 3 three bf16 planes — the form IN USE (the
 *                        config's trailing int 21 selects it; an fp16-pair engine whose weights exceed the fp16 range at load,
 *                        or whose activations do during a call, has switched itself to 3); -1 for 16-bit engines
 *   "saturation_events"  calls on this handle during which a pair operand met the fp16 range limit and that were therefore
 *                        re-run on three bf16 planes (0 or 1: the switch is permanent)
 *   "adaln_fold"         1 when the load-time vectors of the AdaLN fold exist (LayerNorm statistics carried by the GEMM epilogues)
 *   "attn_v_rows"        1 when an fp32 engine's QKV epilogue hands pre-split V to attention as rows like K (the default), 0 when
 *                        transposed (environment MI355TTS_ATTN_V_ROWS=0, or K / V not pre-split)
 * Returns the value, or a negative MI_E* code for a null handle / unknown key.                                              */
int64_t     mi_f5_info(mi_f5* h, const char* key);
/* graph A.  audio (L) int16, text_ids (T) int32 (pad value -1 allowed), max_duration N.
 * noise_in != NULL injects the initial noise (N,100); else it is drawn from `seed`.
 * Outputs (any may be NULL): noise (N,100), rope_cos/rope_sin (N,64) [the ONNX graph broadcasts these
 * to (2,16,N,64) and a transposed K copy], cat_mel_text / cat_mel_text_drop (N,612), ref_signal_len.   */
int         mi_f5_preprocess(mi_f5* h, const int16_t* audio, int64_t L, const int32_t* text_ids, int64_t T,
                             int64_t max_duration, const float* noise_in, uint64_t seed, float* noise,
                             float* rope_cos, float* rope_sin, float* cat_mel_text, float* cat_mel_text_drop,
                             int64_t* ref_signal_len, int mem);
/* unit-level entry (tests): STFT-B of graph A alone (F5_TTS/STFT_Process.py:144-157, reflect padding): audio (L) int16 ->
 * spec (L/hop + 1, 2*(n_fft/2+1)) fp32, row f = [re(0..n_fft/2) | im(0..n_fft/2)] of frame f.                          */
int         mi_f5_stft(mi_f5* h, const int16_t* audio, int64_t L, float* spec, int mem);
/* graph B, one call = `fuse` Euler/CFG steps starting at *time_step (host int); noise (U,N,100) is
 * updated in place, *time_step += fuse.  cat_mel_text(_drop): (U,N,612).                              */
int         mi_f5_transformer_step(mi_f5* h, float* noise, const float* cat_mel_text, const float* cat_mel_text_drop,
                                   int U, int64_t N, int32_t* time_step, int fuse, int mem);
/* the whole NFE loop on device: steps k0 .. k0+n_steps-1 (reference: k0 = 0, n_steps = nfe_step-1)   */
int         mi_f5_sample(mi_f5* h, float* noise, const float* cat_mel_text, const float* cat_mel_text_drop, int U,
                         int64_t N, int k0, int n_steps, int mem);
/* tests: one DiT evaluation at grid index k -> pred (2U, N, 100) (cond branch first)                 */
int         mi_f5_dit_eval(mi_f5* h, const float* noise, const float* cat_mel_text, const float* cat_mel_text_drop,
                           int U, int64_t N, int k, float* pred, int mem);
/* graph C.  denoised (U,N,100), ref_signal_len R -> int16 (U, (N-R-1)*hop); out_f32 (optional) is the
 * float signal before clamp/int16.  *out_len receives the per-utterance sample count.                 */
int         mi_f5_decode(mi_f5* h, const float* denoised, int U, int64_t N, int64_t ref_signal_len, int16_t* out,
                         float* out_f32, int64_t* out_len, int mem);
/* A -> loop -> C without leaving the device.  audio (U,L), text_ids (U,T), noise_in (U,N,100) or NULL. */
int         mi_f5_synthesize(mi_f5* h, int U, const int16_t* audio, int64_t L, const int32_t* text_ids, int64_t T,
                             int64_t max_duration, const float* noise_in, uint64_t seed, int16_t* out,
                             int64_t* out_len, int mem);

/* A -> loop, with the generated frames handed on as a vocoder mel instead of going through Vocos: mel_out (U, 100, N - R)
 * fp32, channels first = the `mel_features` layout of mi_bigvgan_forward (BigVGAN-v2 24khz_100band_256x has F5's 100 bands,
 * hop 256, 24 kHz).  The "F5-TTS + BigVGAN" pipeline of BASELINE.json's metric; the reference's bigvgan-type mel front end is
 * F5_TTS/modeling_modified/F5/modules.py:30-72 (its exported graphs use the Vocos pair).  *n_frames receives N - R.     */
int         mi_f5_synthesize_mel(mi_f5* h, int U, const int16_t* audio, int64_t L, const int32_t* text_ids, int64_t T,
                                 int64_t max_duration, const float* noise_in, uint64_t seed, float* mel_out,
                                 int64_t* n_frames, int mem);

/* Ragged batch: U utterances, each with its own prompt audio (audio_lens[u] samples), text (text_lens[u] ids) and
 * max_duration N_u (max_durations[u]), through graph A, the sampling loop (one hipGraph) and graph C in one call.
 * audio, text_ids and noise_in are the per-utterance arrays concatenated (noise_in: sum N_u x 100, or NULL to draw utterance
 * u's noise with seed + u, as mi_f5_synthesize does); data arrays follow `mem`, the length arrays are always host int64.
 * The loop runs on padded slabs of Nmax = max N_u rows (utterance u owns slab u; rows >= N_u stay zero and never reach a live
 * row): each utterance gets the waveform it gets alone.  out receives the int16 waveforms concatenated, out_lens[u] =
 * (N_u - R_u - 1) * hop with R_u the prompt's frames.  MI_EINVAL, with the handle still usable, for U < 1, N_u < R_u + 1,
 * N_u < T_u, N_u > max_signal_length, out_cap below the sum of out_lens, or a text id out of range in any utterance.   */
int         mi_f5_synthesize_ragged(mi_f5* h, int U, const int16_t* audio, const int64_t* audio_lens, const int32_t* text_ids,
                                    const int64_t* text_lens, const int64_t* max_durations, const float* noise_in, uint64_t seed,
                                    int16_t* out, int64_t out_cap, int64_t* out_lens, int mem);
/* The same ragged batch handed on as mels for a vocoder engine: utterance u's generated frames [R_u, N_u) leave as (100, N_u - R_u)
 * fp32 channels first, concatenated in mel_out (mel_cap floats) — exactly the `mel` of mi_bigvgan_forward_ragged, whose frames
 * are n_frames[u] = N_u - R_u (host int64).  Inputs and checks as mi_f5_synthesize_ragged.                                   */
int         mi_f5_synthesize_mel_ragged(mi_f5* h, int U, const int16_t* audio, const int64_t* audio_lens, const int32_t* text_ids,
                                        const int64_t* text_lens, const int64_t* max_durations, const float* noise_in, uint64_t seed,
                                        float* mel_out, int64_t mel_cap, int64_t* n_frames, int mem);
/* tests: one DiT evaluation of a ragged batch at grid index k.  noise (U, Nmax, 100), cat_mel_text(_drop) (U, Nmax, 612) in
 * the padded layout (rows >= lens[u] are ignored), lens host int64 in [1, Nmax] -> pred (2U, Nmax, 100), cond branch first;
 * only rows < lens[u] of items 2u, 2u + 1 are defined.                                                                  */
int         mi_f5_dit_eval_ragged(mi_f5* h, int U, const int64_t* lens, const float* noise, const float* cat_mel_text,
                                  const float* cat_mel_text_drop, int64_t Nmax, int k, float* pred, int mem);

/* ---- IndexTTS acoustic GPT-2 (graphs B, C, E + the greedy decode loop) ------------------------------------------
 * Replaces ort_session_B / _C / _E of IndexTTS/Inference_IndexTTS_ONNX.py:619-675 and the loop at :745-783
 * (graph definitions: IndexTTS/Export_IndexTTS.py:203-289).  The KV cache lives in the handle (the reference
 * passes 2*layers growing tensors in and out of every call); mi_gpt_kv_read / _write expose it in the reference's
 * tensor layouts.  cfg = {hidden, layers, heads, inner, mel_codes, text_tokens, max_mel_pos, max_text_pos, max_seq
 * [, max_batch = 1]}, 1 <= max_batch <= 64 (mi_gpt_create* returns NULL with mi_last_error set otherwise).  Every slot has its own
 * KV cache, 2 * layers * hidden * max_seq elements of the engine dtype: 126 MB per slot at IndexTTS-1.5 size with max_seq =
 * 1024 in f16, 8.05 GB at 64 slots; an allocation that fails is reported by mi_gpt_create* like any other error.
 * weights: canonical fp32 blob of mi355tts.weights.pack_gpt (Conv1D weights transposed to (out, in); q and k rows
 * pre-scaled by head_dim^-0.25 like Export_IndexTTS.py:257-258).                                                  */
typedef struct mi_gpt mi_gpt;
typedef struct mi_cond mi_cond;
int64_t     mi_gpt_param_count(const int32_t* cfg, int n_cfg);
mi_gpt*     mi_gpt_create(const int32_t* cfg, int n_cfg, const float* weights, int64_t n_weights, int dtype, int device);
mi_gpt*     mi_gpt_create_mem(const int32_t* cfg, int n_cfg, const float* weights, int64_t n_weights, int dtype, int device,
                              int mem);
void        mi_gpt_destroy(mi_gpt* h);
/* Per-channel uint8 weights, dequantised in the kernels.  The six matrix kinds of the blob (c_attn, attn.c_proj, c_fc, mlp.c_proj of
 * every layer and lm_head.1, stored as (n, k) rows) are held as bytes; everything else (embeddings, position tables, LayerNorm vectors,
 * biases: fp32; KV cache: the engine dtype) is as in mi_gpt_create.  The format, per output row n, all in float32:
 *     rmin = min(0, min_k w[n,k]), rmax = max(0, max_k w[n,k]); scale[n] = (rmax - rmin) / 255 (an all-zero row: scale 1, zp 0);
 *     zp[n] = clip(rint(-rmin / scale), 0, 255); q[n,k] = clip(rint(w[n,k] / scale) + zp, 0, 255); dq[n,k] = float32(q - zp) * scale
 * (rint: round half to even).  It restates the weight side of the reference's int8 export (IndexTTS/Optimize_ONNX.py:
 * quantize_dynamic(per_channel=True, weight_type=QUInt8, MatMulConstBOnly=True), reduce_range off); parity with onnxruntime's own bytes
 * is not pinned by any test.  Unlike that export the activations are NOT quantised: weights 8-bit, activations 16-bit.  The kernels
 * compute act(scale[n] * sum_k (q - zp) x'[k] + bias[n]) + res[n] with (q - zp) exact and the sum in fp32; prompt passes of two or
 * more rows read an f16 copy f16(dq) of the matrix in use, written into one scratch of the handle.
 *   mi_gpt_quantize_u8   the rule above on the host (no GPU needed): w (n, k) -> q (n, k), scale (n), zp (n).
 *   mi_gpt_create_q8     mi_gpt_create_mem on the same canonical fp32 blob (host or device by `mem`), quantised at creation: the same
 *                        bytes whichever `mem`.  dtype must be MI_F16; MI_F32 and MI_BF16 are refused (NULL, mi_last_error names the
 *                        cause), as are a hidden or inner that is not a multiple of 16.  "gpt_mfma_min" and MI355TTS_GPT_NO_MFMA apply.
 *   mi_gpt_weight_bytes  device bytes the handle holds for the six matrix kinds.  A q8 handle: sum n * k (bytes) + 4 * sum n (scales)
 *                        + sum n (zero points) + 2 * max n * k (the prompt scratch); any other handle: sum n * k elements of its dtype. */
int         mi_gpt_quantize_u8(const float* w, int n, int k, uint8_t* q, float* scale, uint8_t* zp);
mi_gpt*     mi_gpt_create_q8(const int32_t* cfg, int n_cfg, const float* weights, int64_t n_weights, int dtype, int device, int mem);
int64_t     mi_gpt_weight_bytes(mi_gpt* h);
/* graph B: text_ids (n) -> text_hidden_state (n + 2, hidden): start id 0 / end id 1 added, + position rows. */
int         mi_gpt_text_embed(mi_gpt* h, const int32_t* text_ids, int n, float* out, int mem);
/* graph C: mel embedding of gpt_id + mel position row gen_len -> (hidden). (the caller keeps gen_len + 1) */
int         mi_gpt_mel_embed(mi_gpt* h, int32_t gpt_id, int64_t gen_len, float* out, int mem);
/* history_len := 0 (the reference re-feeds the empty init_past_keys_E / init_past_values_E, :796-800) */
int         mi_gpt_reset(mi_gpt* h);
int64_t     mi_gpt_history_len(mi_gpt* h);
/* graph E: hidden_state (ids_len, hidden) appended after the handle's history; repeat_penality (mel_codes) or NULL
 * (= ones); attention_mask 1 for the prompt pass, 0 for single-token steps.  Outputs: last_hidden_state (hidden),
 * max_logit_id (1), optionally the logits before the penalty multiply (mel_codes).  history_len += ids_len.     */
int         mi_gpt_step(mi_gpt* h, const float* hidden_state, int ids_len, const float* repeat_penality,
                        int attention_mask, float* last_hidden_state, int32_t* max_logit_id, float* logits, int mem);
/* in_key_i / in_value_i / out_key_i / out_value_i of graph E: keys (heads, 64, history), values (heads, history, 64).
 * mi_gpt_kv_write sets history_len := hist (write every layer with the same hist). */
int         mi_gpt_kv_read(mi_gpt* h, int layer, float* keys, float* values, int mem);
int         mi_gpt_kv_write(mi_gpt* h, int layer, const float* keys, const float* values, int hist, int mem);
/* The per-sentence loop (:745-783) on the device: prompt (P, hidden) = graph D's concat; at most max_new tokens
 * (the reference's generate_limit = MAX_GENERATE_LENGTH - P); stops after a token in stop_ids; repeat_value /
 * penalty_range = REPEAT_PENALITY / PENALITY_RANGE.  repeat_penality (mel_codes) is read and written back (the
 * reference carries it across sentences, :685) — NULL starts from ones.  Outputs: tokens (max_new), hidden
 * (max_new, hidden) = the stacked last_hidden_state rows graph F consumes, *n_out (host) = tokens produced.     */
int         mi_gpt_generate(mi_gpt* h, const float* prompt, int P, int max_new, const int32_t* stop_ids, int n_stop,
                            float repeat_value, int penalty_range, float* repeat_penality, int32_t* tokens,
                            float* hidden, int32_t* n_out, int mem);

/* The same loop for nb sentences at once (nb <= the handle's max_batch = optional 10th cfg int): prompt passes run one
 * after the other, then every decode step serves all unfinished sentences with ONE pass over the weights (batched
 * GEMV), each sentence with its own cache, history, penalty vector, stop test and limit.  prompts = the nb prompts
 * concatenated row-wise (sum(prompt_rows), hidden); prompt_rows / max_new / n_out are host arrays of nb ints;
 * repeat_penality (nb, mel_codes) in/out or NULL; tokens (nb, cap), hidden (nb, cap, hidden).  Results per sentence
 * are identical to mi_gpt_generate on that sentence alone (fp32: bit-for-bit the same kernels' arithmetic order).
 *
 * nb may be anything up to max_batch <= 64.  Up to 16 sentences a decode-step linear layer is one launch of the batched GEMV or
 * of the 16-column matrix-core kernel.  Above 16:
 *   - 16-bit engines, wherever the matrix-core kernel would serve 16 sentences (option "gpt_mfma" set, nb >= "gpt_mfma_min", K
 *     splitting into 64-wide blocks per wave): ONE launch whose weight fragments feed ceil(nb / 16) column tiles.  Slot
 *     independence: the MFMAs that accumulate one (weight row, sentence) output are the 16-column kernel's in its order, so a
 *     sentence's result does not depend on its slot or on nb — column c is bit for bit column c % 16 of the 16-column kernel.
 *   - everything else (fp32 engines, "gpt_mfma" = 0, a K that does not split): group rule — slots [16g, 16g + 16) form group g
 *     and each group runs the launch it would run as a batch of its own size, the weights streamed once per group.  This is
 *     the correctness path, not a fast one: a wide fp32 batch gives exactly what its index-order groups of 16 give. */
int         mi_gpt_generate_batch(mi_gpt* h, int nb, const float* prompts, const int32_t* prompt_rows,
                                  const int32_t* max_new, const int32_t* stop_ids, int n_stop, float repeat_value,
                                  int penalty_range, float* repeat_penality, int32_t* tokens, float* hidden, int cap,
                                  int32_t* n_out, int mem);

/* ---- sampling: seeded temperature / top-k / top-p choice of the mel code, on the device ------------------------------------
 * The reference decodes greedily and so do the entries above; these are the engine's own.  Each sentence has
 * temperature > 0, top_k >= 0, top_p in (0, 1] and a 64-bit seed.  For decode index n (the number of tokens the sentence has
 * produced before this one; n = 0 is the token of the prompt pass) the token is chosen from the step's logits as follows.
 *   1. z[c] = (logits[c] * pen[c]) * inv_T in fp32, inv_T = 1.0f / temperature computed once on the host in fp32.  The
 *      penalty multiply is the reference's (its quirk on negative logits included).  Two multiplies, no add: nothing
 *      contracts to an FMA and z is bit-reproducible in numpy float32.
 *   2. top-k: t_k = the k-th largest value of z counted with multiplicity, K = {c : z[c] >= t_k} (ties at the threshold
 *      are all kept).  top_k == 0 or top_k >= codes: K = every code.
 *   3. e[c] = exp(z[c] - max z) for c in K, S = sum of e over K.
 *   4. top-p: t_p = the largest value v taken by z on K for which sum{e[c] : c in K, z[c] >= v} >= top_p * S;
 *      P = {c in K : z[c] >= t_p}: the smallest set of most probable codes that reaches the mass, closed under ties; it
 *      always holds the argmax.  top_p >= 1: P = K.
 *   5. u = (w0 >> 8) * 2^-24 in [0, 1), w0 = the first output word of Philox4x32-10 with key (seed & 0xffffffff, seed >> 32)
 *      and counter (n, 0, 0, 0) (mi_gpt_sample_logits: (n & 0xffffffff, n >> 32, 0, 0)).  The token is the first c of P in
 *      ascending index order with sum{e[c'] : c' in P, c' <= c} > u * S_P, S_P = sum of e over P; the last index of P should
 *      rounding leave none.  (The CDF runs in index order, not probability order: the same distribution, and no sort.)
 *   6. top_k == 1 is greedy exactly: argmax of logits * pen, lowest index on ties, no draw: the tokens of mi_gpt_generate.
 * The device evaluates e as 2^-40 fixed point and sums integers, so the choice does not depend on the order of any sum: with the
 * counter the sentence's own decode index and the key its own seed, the tokens do not depend on the slot, the batch size,
 * the host's 16-step chunking, or eager launch versus graph replay.  Everything after the choice (token store, stop test,
 * penalty update and reset, limit, last_hidden_state row) is the greedy entries', unchanged.  Handles with more than 16384
 * mel codes cannot sample (MI_EINVAL).
 *
 * mi_gpt_generate_sampled = mi_gpt_generate + the sentence's parameters; mi_gpt_generate_batch_sampled =
 * mi_gpt_generate_batch + host arrays of nb parameters (an item with top_k == 1 decodes greedily).  MI_EINVAL, with the
 * handle still usable, for temperature <= 0 or not finite, top_k < 0, top_p outside (0, 1] or not finite.               */
int         mi_gpt_generate_sampled(mi_gpt* h, const float* prompt, int P, int max_new, const int32_t* stop_ids, int n_stop,
                                    float repeat_value, int penalty_range, float* repeat_penality, int32_t* tokens,
                                    float* hidden, int32_t* n_out, int mem, float temperature, int top_k, float top_p,
                                    uint64_t seed);
int         mi_gpt_generate_batch_sampled(mi_gpt* h, int nb, const float* prompts, const int32_t* prompt_rows,
                                          const int32_t* max_new, const int32_t* stop_ids, int n_stop, float repeat_value,
                                          int penalty_range, float* repeat_penality, int32_t* tokens, float* hidden, int cap,
                                          int32_t* n_out, int mem, const float* temperature, const int32_t* top_k,
                                          const float* top_p, const uint64_t* seeds);
/* unit-level entry (tests, no handle): the same device code on rows of logits.  logits (rows, codes), pen (rows, codes) or
 * NULL (= ones), 1 <= codes <= 16384; temperature / top_k / top_p / seeds / positions (= n) are HOST arrays of `rows`
 * entries; tokens (rows), u_out (rows) = the u of step 5, prob_out (rows, codes) or NULL = e[c] / S_P on P and 0 elsewhere
 * (top_k == 1: 1 at the token) follow `mem` like logits and pen.                                                        */
int         mi_gpt_sample_logits(const float* logits, const float* pen, int rows, int codes, const float* temperature,
                                 const int32_t* top_k, const float* top_p, const uint64_t* seeds, const int64_t* positions,
                                 int32_t* tokens, float* u_out, float* prob_out, int mem);

/* ---- beam search: num_beams hypotheses per sentence over one shared KV cache, on the device ------------------------------------
 * The scheme of upstream IndexTTS's third knob (it runs 3 beams) in its simplest exact form.  One sentence runs with
 * B = num_beams hypotheses in B consecutive slots; its starting penalty vector is pen0.
 *   Selection 0.  The one prompt pass gives logits L.  z[c] = L[c] * pen0[c] in fp32 (one multiply: the reference's penalty,
 *      its quirk on negative logits included), lp[c] = z[c] - lse(z), lse(z) = m + log(sum exp(z - m)), m = max z.  Hypotheses
 *      0..B-1 are the B codes of largest lp in descending order, a tie going to the lower code; score_b = lp[c_b].
 *   Selection n >= 1.  Every hypothesis b runs one decode step (graph C of its last token at gen_len = n, keys and values of
 *      its own history) that gives L_b; z_b = L_b * pen_b, cand(b, c) = score_b + (z_b[c] - lse(z_b)).  The new hypotheses
 *      0..B-1 are the B largest candidates over all B * codes in descending order, a tie going to the lower flat index
 *      b * codes + c.  New hypothesis i = (parent b_i, code c_i) takes score = cand and inherits everything from its parent:
 *      token history, KV history, penalty vector, reset index, last_hidden_state rows.  It then does the greedy loop's
 *      bookkeeping with its own token: token store, penalty write, reset over penalty_range.
 *   End.  The sentence is done after selection n when hypothesis 0's token is a stop id or n + 1 == max_new; the stop token is
 *      stored and counted and, as in the greedy loop, not penalised.  The result is hypothesis 0: its n + 1 tokens, its n + 1
 *      last_hidden_state rows (row n = the row of the forward pass whose logits produced token n, on that hypothesis' own
 *      path: what graph F consumes), its score, and its penalty vector written back to repeat_penality.
 *   Property: a hypothesis other than 0 that emits a stop id stays an ordinary hypothesis — the token is stored and penalised
 *      like any other and the hypothesis keeps decoding.  There is no pool of finished hypotheses and no length penalty
 *      (upstream's default is 0).
 *   num_beams == 1 is greedy exactly: the argmax of z, lowest index on ties, the choice not passing through lse: the tokens
 *      and rows of mi_gpt_generate_batch.
 * Scores are fp32 and the order of the sum inside lse is the implementation's (fixed: the same bits from every launch, slot,
 * batch and graph replay), so scores hold to a tolerance against another evaluation order and the choice holds wherever
 * rounding cannot decide.  Nothing is copied when hypotheses change slots: cache rows written so far never change, so the
 * prompt's keys and values are stored once per sentence (in the group's first slot) and every later position is read from the
 * slot a small per-hypothesis ancestor table names.  Beams and sampling do not combine here: this search is deterministic
 * (the pool mode below draws).
 *
 * MI_EINVAL, with the handle still usable: num_beams < 1 or > 8, nb * num_beams above the handle's max_batch (<= 64: a
 * group of hypotheses may lie across a 16-slot boundary, the decode linears do not know about groups), num_beams >
 * mel_codes, and what mi_gpt_generate_batch rejects.
 *
 * nb sentences, each with num_beams hypotheses in num_beams consecutive slots; arguments as mi_gpt_generate_batch;
 * scores (nb) or NULL = hypothesis 0's cumulative log-probability; repeat_penality (nb, mel_codes) in/out or NULL. */
int         mi_gpt_generate_beam(mi_gpt* h, int nb, const float* prompts, const int32_t* prompt_rows, const int32_t* max_new,
                                 const int32_t* stop_ids, int n_stop, float repeat_value, int penalty_range,
                                 float* repeat_penality, int num_beams, int32_t* tokens, float* hidden, int cap, int32_t* n_out,
                                 float* scores, int mem);
/* unit entry (tests, no handle): one selection on rows of logits.  logits, pen (or NULL = ones): (groups*beams, codes);
 * prev_scores (groups*beams); first != 0: selection 0 (only row g*beams of each group is read, prev_scores ignored).
 * Outputs (groups*beams): parents (row inside the group), tokens, scores.  1 <= codes <= 16384, 1 <= beams <= 8,
 * beams <= codes. */
int         mi_gpt_beam_select(const float* logits, const float* pen, const float* prev_scores, int groups, int beams, int codes,
                               int first, int32_t* parents, int32_t* tokens, float* scores, int mem);

/* ---- beam search with a finished pool, and beam sampling: the second, opt-in beam mode ("pool" mode) ----------------------------
 * What upstream IndexTTS asks of generate() (num_beams = 3, do_sample, top_k = 30, top_p = 0.8, length_penalty = 0): finished
 * hypotheses are kept aside, the search goes on while a running one can still beat them, the best of the pool is returned, and
 * the candidates may be drawn.  It follows transformers' _beam_search for one sentence; the entries above keep their results.
 * One sentence has B = num_beams hypotheses in B consecutive slots, a stop set of n_stop ids, a limit max_new, a starting penalty
 * vector pen0, length_penalty (float), early_stopping (0 or 1) and optionally a sampling record (temperature, top_k, top_p, seed).
 * K = (n_stop + 1) * B candidates are kept per selection (transformers' beams_to_keep): B of them are sure not to stop.
 * State: running scores s_0 .. s_{B-1} (fp32); a pool of B entries (score, initially -1e9; a finished flag; length, tokens and
 * ancestry); one flag `open`, initially true.  Selection n (n = 0 reads only row 0 of the prompt pass, as above):
 *   1. z = L * pen (one rounded fp32 multiply, as above), lp = z - lse(z).
 *   2. Warp.  Deterministic mode: w = lp.  Sampling mode: w = lp * inv_T (transformers' order: the temperature on
 *      log-probabilities, not renormalised), then top-k and top-p per row by steps 2-4 of "sampling" applied to w, except that
 *      the K best codes of a row (ties to the lower code) are always kept: min_tokens_to_keep = K.  (transformers uses
 *      n_stop + 1, which can leave fewer candidates than it draws and then raises.)  Codes outside get -inf.
 *   3. acc(b, c) = s_b + w_b[c]; flat index i = b * codes + c.
 *   4. Candidates, in "candidate order".  Deterministic: the K largest acc, descending, ties to the lower i.  Sampling:
 *      key(i) = acc(i) + g(i), g = -log(-log u), u = ((word >> 8) + 0.5) * 2^-24, word = output word (i & 3) of Philox4x32-10
 *      with the sentence's seed as key and counter (n, i >> 2, 1, 0) (the 1 keeps the stream apart from the sampler's
 *      (n, 0, 0, 0)); the K largest keys, descending, ties to the lower i.  This is Gumbel-top-K: exactly K draws without
 *      replacement from softmax(acc), in draw order, which is what torch.multinomial(softmax(acc), K) does; no renormalised
 *      sequential pass, and the choice does not depend on any summation order.
 *   5. stop(i): the candidate's code is a stop id, or n + 1 == max_new.
 *   6. Next running hypotheses: the B candidates of largest acc among those with stop false, descending, ties to the earlier
 *      candidate.  They inherit from their parent exactly as above (penalty vector, reset index, KV and token history, rows)
 *      and do the greedy loop's bookkeeping with their own token; a running hypothesis never holds a stop id.
 *   7. Pool.  Only while `open`, and not (early_stopping and every pool entry finished): each of the first B candidates in
 *      candidate order with stop true enters at score acc / (n + 1)^length_penalty.  The pool keeps the B best of old and new,
 *      an old entry before a new one on ties, then candidate order.  An entry freezes its parent's history plus its own token.
 *   8. If every pool entry is finished: open := open and s'_0 / (n + 1)^length_penalty > the lowest pool score (s'_0: the best
 *      new running score).  Otherwise `open` is unchanged.
 *   9. The sentence ends after selection n when `open` is false, or early_stopping is set and every pool entry is finished, or
 *      n + 1 == max_new.
 * The result is pool entry 0: its tokens (the stop id stored and counted as above), its last_hidden_state rows along its own
 * path (row n = the row of the pass whose logits produced token n) and its score.  repeat_penality is read and not written
 * back: pool entries keep no vector.  The penalty stays the engine's (logits * pen before the log-softmax, with its range
 * reset); transformers' RepetitionPenaltyLogitsProcessor is not part of this, and early_stopping = "never" is not offered.
 *   Property: B = 1, deterministic, length_penalty = 0 gives the tokens of mi_gpt_generate wherever rounding cannot decide a
 *      selection.
 * Scores hold to a tolerance and choices wherever rounding cannot decide, as above; sampled results are the same bits from
 * every launch, slot, batch and graph replay.  Pool mode through the sentence queue, as a session and streamed:
 * mi_gpt_generate_queue_beam_pool / mi_gpt_queue_begin_beam_pool, below beside "beam search through the sentence queue" (a
 * group's retirement there follows the frozen list).
 *
 * MI_EINVAL, before anything is launched and with the handle still usable: what mi_gpt_generate_beam rejects; K > 64 or
 * K > mel_codes; length_penalty not finite; early_stopping outside {0, 1}; an invalid sampling record; top_k not 0 and below K;
 * more than 16384 mel codes with sampling; only some of the four sampling arrays.
 *
 * mi_gpt_generate_beam_pool: the arguments of mi_gpt_generate_beam (repeat_penality (nb, mel_codes) or NULL, read only), then
 * length_penalty, early_stopping and four HOST arrays of nb sampling parameters (all four NULL: deterministic).  scores (nb) or
 * NULL = the returned entry's score (0 for a sentence with max_new == 0, which returns nothing). */
int         mi_gpt_generate_beam_pool(mi_gpt* h, int nb, const float* prompts, const int32_t* prompt_rows, const int32_t* max_new,
                                      const int32_t* stop_ids, int n_stop, float repeat_value, int penalty_range,
                                      const float* repeat_penality, int num_beams, float length_penalty, int early_stopping,
                                      const float* temperature, const int32_t* top_k, const float* top_p, const uint64_t* seeds,
                                      int32_t* tokens, float* hidden, int cap, int32_t* n_out, float* scores, int mem);
/* unit entry (tests, no handle): one selection of one sentence with the whole state passed in and out.  logits, pen (or NULL =
 * ones): (beams, codes), following `mem`; everything else is a HOST array.  prev_scores (beams; ignored at n == 0);
 * pool_scores / pool_finished (beams) and *open in / out; temperature / top_k / top_p / seed point to one value each (all four
 * NULL: deterministic).  Outputs: cand / cand_acc / cand_stop (K = (n_stop + 1) * beams) = flat index, acc and stop flag in
 * candidate order; parents / tokens / scores (beams) = the next running hypotheses (-1 where no live candidate is left);
 * pool_src (beams): -1 - j = the entry that was at place j, q >= 0 = candidate q; *done = step 9.  1 <= codes <= 16384,
 * 0 <= n < max_new, K <= 64 and <= codes. */
int         mi_gpt_beam_pool_select(const float* logits, const float* pen, const float* prev_scores, int beams, int codes, int n,
                                    int max_new, const int32_t* stop_ids, int n_stop, float* pool_scores, int32_t* pool_finished,
                                    int32_t* open, float length_penalty, int early_stopping, const float* temperature,
                                    const int32_t* top_k, const float* top_p, const uint64_t* seed, int32_t* cand, float* cand_acc,
                                    int32_t* cand_stop, int32_t* parents, int32_t* tokens, float* scores, int32_t* pool_src,
                                    int32_t* done, int mem);

/* unit entries (tests, no handle): ONE launch of each of the GPT's four attention kernels, through the launcher the engine
 * calls (same kernel, grid, block and dynamic LDS).  softmax(q K^T [+ mask]) V per head of 64 columns, no scale (the engine's q
 * is pre-scaled by the folded weights).  qkv (rows, 3 * hidden), hidden = 64 * heads, of which only the q third is read; kc /
 * vc: K and V caches in the engine's layout [slot][head][max_seq][64]; out (rows, hidden).  All fp32 and following `mem`; the
 * inputs are rounded to `dtype` (MI_F32 | MI_F16 | MI_BF16) on the device, the output widened back (exact).  The integer tables
 * are HOST arrays.  1 <= heads <= 64, 1 <= max_seq <= 8192, 1 <= nslots <= 64.  A cache row the launch must not read may hold
 * anything, NaN included.
 *   decode       row r = slot r attends to keys 0 .. kv-1 of its own slot, kv = min(hist[r] + 1, max_seq); 0 <= hist <= max_seq.
 *   decode_beam  slots in groups of `beams` (1..8, dividing nslots).  P = hist - ndec + 1 (0 <= ndec <= hist + 1): key j < P is
 *                read from the group's first slot, key P + n from slot anc[ndec & 1][r][n] of the group; anc (2, nslots,
 *                max_seq), every entry in [0, beams).
 *   prompt       ONE slot (kc / vc: [head][max_seq][64]) holding hist + rows keys; row i of the `rows` new ones sees all of
 *                them, key j > i (j absolute, i inside the new block) with -128 * flag added; hist + rows <= max_seq.
 *   prompt_packed  segs (nseg, 3) = (first, rows, slot): ascending, gap-free, distinct slots, the rows summing to total <=
 *                max_seq; packed row first + i of a segment is row i of a prompt of `rows` rows in `slot`, history 0, mask on. */
int         mi_gpt_attn_decode(const float* qkv, const float* kc, const float* vc, int dtype, int heads, int max_seq, int nslots,
                               const int32_t* hist, float* out, int mem);
int         mi_gpt_attn_decode_beam(const float* qkv, const float* kc, const float* vc, int dtype, int heads, int max_seq,
                                    int nslots, const int32_t* hist, const int32_t* ndec, int beams, const int32_t* anc, float* out,
                                    int mem);
int         mi_gpt_attn_prompt(const float* qkv, const float* kc, const float* vc, int dtype, int heads, int max_seq, int hist,
                               int rows, int flag, float* out, int mem);
int         mi_gpt_attn_prompt_packed(const float* qkv, const float* kc, const float* vc, int dtype, int heads, int max_seq,
                                      int nslots, const int32_t* segs, int nseg, int total, float* out, int mem);

/* unit entries (tests, no handle): ONE launch of a decode-step linear layer of the GPT, through the launchers the engine calls
 * (csrc/gpt.h launch_gpt_gemv / launch_gpt_gemv_b: same dispatch, kernel and grid).  out = act(w x' + bias) + res.  Arrays are
 * fp32 and follow `mem`; w (n, k), x and the caches are rounded to `dtype` (MI_F32 | MI_F16 | MI_BF16) on the device, outputs are
 * widened back (exact); bias, res and the LayerNorm vectors stay fp32, as in the engine.  hist is a HOST value / array.  act: 0 or
 * 1 (gelu_new).  out_f32 != 0: the launch stores fp32, otherwise `dtype`.  `out` and `pre_out` are preset to NaN bytes on the
 * device, so an element the launch does not write comes back NaN.  k a multiple of 8, at most 16384; bias, res may be NULL.
 *   decode  one row: x (k), out (n), res (n).  ln_w, ln_b (k) given: x stays fp32 and x' = LayerNorm(x), eps 1e-5 (k <= 2048 at
 *           MI_F32, <= 4096 at 16 bits; no res).  pre_w, pre_b (k, with ln_w; k <= 2048): x' = LayerNorm(LayerNorm_pre(x)), the
 *           inner row also to pre_out (k) or NULL.  qkv != 0 (with ln_w, n == 3 * k, k a multiple of 64): columns [k, 3k) go to row
 *           `hist` of kc then vc — ONE layer's caches [k / 64][max_seq][64], in and out — when hist < max_seq, and not to out;
 *           0 <= hist <= max_seq <= 8192.
 *   batch   nb rows (1..64): x (nb, k), res (nb, n), hist[nb], kc / vc [nb][k / 64][max_seq][64] in and out (qkv needs no
 *           LayerNorm here).  The device x array has the engine's padded row count P = mi_gpt_linear_batch_rows(nb) (2, 4, 8, then
 *           multiples of 16); rows nb .. P-1 are copies of x_dead (k), zeros if NULL.  out (P, n): rows >= nb are never written. */
int         mi_gpt_linear_decode(const float* w, const float* bias, const float* x, int dtype, int n, int k, const float* ln_w,
                                 const float* ln_b, const float* pre_w, const float* pre_b, float* pre_out, const float* res,
                                 int act, int out_f32, int qkv, int hist, int max_seq, float* kc, float* vc, float* out, int mem);
int         mi_gpt_linear_batch(const float* w, const float* bias, const float* x, const float* x_dead, int dtype, int n, int k,
                                int nb, const float* res, int act, int out_f32, int qkv, const int32_t* hist, int max_seq,
                                float* kc, float* vc, float* out, int mem);
int         mi_gpt_linear_batch_rows(int nb);       /* P above; < 0 (MI_EINVAL) outside 1..64 */
/* the same two entries on uint8 weights (the format of mi_gpt_create_q8): q (n, k) bytes, scale (n) fp32, zp (n) bytes in place of w,
 * following `mem`; dtype is the activation type and must be MI_F16; k a multiple of 16, at most 8192 in decode, and the fused LayerNorm
 * takes k <= 4096.  Same NaN presets, same launchers as the engine (csrc/gpt_q8.hip). */
int         mi_gpt_linear_decode_q8(const uint8_t* q, const float* scale, const uint8_t* zp, const float* bias, const float* x,
                                    int dtype, int n, int k, const float* ln_w, const float* ln_b, const float* pre_w,
                                    const float* pre_b, float* pre_out, const float* res, int act, int out_f32, int qkv, int hist,
                                    int max_seq, float* kc, float* vc, float* out, int mem);
int         mi_gpt_linear_batch_q8(const uint8_t* q, const float* scale, const uint8_t* zp, const float* bias, const float* x,
                                   const float* x_dead, int dtype, int n, int k, int nb, const float* res, int act, int out_f32,
                                   int qkv, const int32_t* hist, int max_seq, float* kc, float* vc, float* out, int mem);

/* ---- sentence queue: any number of sentences through the handle's slots, a slot refilled as soon as its sentence stops ---------
 * A decode step costs little more for 16 live slots than for 1, and 64 cost far less than four times 16,
 * so throughput is the number of LIVE slots.  mi_gpt_generate_batch takes
 * at most max_batch sentences and keeps a finished slot running as a no-op until the longest one ends; this entry takes n >= 1
 * sentences (n is not bound by max_batch), refills a slot when its sentence stops, and runs the prompts of all sentences
 * admitted together as ONE packed pass over the weights (one LayerNorm / linear launch per layer over all their rows; the KV
 * scatter and the causal attention keep every sentence in its own slot, with the reference's additive -128 mask).
 *
 * prompts / prompt_rows / max_new / stop_ids / repeat_value / penalty_range / tokens (n, cap) / hidden (n, cap, hidden) / n_out
 * (host, n) / mem: as mi_gpt_generate_batch.  temperature / top_k / top_p / seeds: HOST arrays of n entries, all four NULL
 * (greedy) or all four given (as mi_gpt_generate_batch_sampled).  There is NO repeat_penality argument: every sentence starts
 * from a penalty vector of ones — the sentences run concurrently, so the reference's carry of the vector from one sentence to
 * the next (:685) has no meaning here.  Per sentence the result is what mi_gpt_generate_batch gives for that sentence from a ones
 * vector: the decode steps are the same launches; the prompt pass differs from the one-by-one pass in GEMM tiling only (fp32:
 * summation order).  A sampled sentence's draws depend on its seed and decode index alone, as everywhere.
 *
 * Validation is mi_gpt_generate_batch's, per sentence (prompt_rows >= 1, 0 <= max_new <= cap, prompt_rows + max_new - 1 <=
 * max_seq, max_new <= the mel position table, at most 6 stop ids, valid sampling parameters, the four arrays together), all of
 * it before anything is launched: MI_EINVAL, with the handle still usable.
 *
 * Scheduling policy (mi355tts.indextts.queue_schedule is its host model; stats counts what it did).  S = min(max_batch, n)
 * slots (max_batch <= 64, so a pass packs up to 64 prompts); sentences are admitted in index order; a sentence with max_new == 0 takes no slot and has n_out = 0.
 *   1. Admit.  While a slot is free and a sentence waits, form a pass: the next waiting sentence takes the lowest free slot,
 *      again and again until no slot is free, nothing waits, or the next sentence's rows would push the pass past max_seq
 *      packed rows (the prompt scratch).  The first sentence of a pass always fits; the pass ends at the first sentence that
 *      does not — nothing behind it is looked at.  The pass runs and gives every admitted sentence its token 0.  Then the
 *      slots' states are read.
 *   2. Retire.  Every slot whose sentence is done (stop id, or max_new tokens — possibly right after its prompt pass) is
 *      retired: its tokens and rows are copied out and the slot is free.  If a slot was freed and a sentence waits: step 1,
 *      with no decode step in between.
 *   3. Finish or decode.  No live slot: finished.  Otherwise c = min(16, min over live slots of (max_new - tokens so far))
 *      batched decode steps over slots 0..S-1 are replayed (finished and empty slots are no-ops), the states are read: step 2.
 * stats (host, 2 ints, or NULL): {sum of the c values = decode steps launched, number of prompt passes}.
 * In the library these three steps are decided by one object, mi::QueuePolicy (csrc/gpt_queue.h), and mi_gpt_queue_schedule
 * (below) drives that same object on the host alone.                                                                    */
int         mi_gpt_generate_queue(mi_gpt* h, int n, const float* prompts, const int32_t* prompt_rows, const int32_t* max_new,
                                  const int32_t* stop_ids, int n_stop, float repeat_value, int penalty_range,
                                  int32_t* tokens, float* hidden, int cap, int32_t* n_out, int mem,
                                  const float* temperature, const int32_t* top_k, const float* top_p, const uint64_t* seeds,
                                  int32_t* stats /* host, 2 ints or NULL: {decode steps launched, prompt passes} */);

/* ---- the sentence queue as a session: the same loop, handed back after every run of decode steps, so that rows can be used
 * (mi_bigvgan_forward_latent_windows) while the queue is still decoding.  mi_gpt_generate_queue IS begin + advance until nothing
 * is left + end over this loop, except for its copy policy (one copy per sentence at retirement, none per round).
 *
 * mi_gpt_queue_begin: arguments and validation of mi_gpt_generate_queue (all of it before anything is launched; MI_EINVAL leaves
 * the handle usable and no session open).  The small host arrays (prompt_rows, max_new, stop ids, sampling parameters) are
 * copied; prompts, tokens (n, cap) and hidden (n, cap, hidden) stay the caller's, follow `mem`, and must live until
 * mi_gpt_queue_end.  Nothing is decoded yet.
 *
 * mi_gpt_queue_advance: ONE round of the policy above: steps 1 and 2 repeated until nothing more can be admitted, then one run
 * of c <= 16 decode steps (step 3) and a look at the states.  Then the caller's arrays are brought up to date: for every live or
 * just-finished sentence i its new tokens and rows [what it had, count[i]) go to tokens[i] and hidden[i].  With mem = MI_DEVICE
 * that is one kernel launch per round over a table of at most 64 (slot, first, count, sentence) entries; with MI_HOST the same
 * kernel packs the rows into a staging buffer and each array leaves in one device-to-host copy.  (A sentence that is retired
 * inside the round before a decode step has run for it, e.g. one whose limit is 1, leaves in a launch of its own ahead of the
 * pass that refills its slot.)  On return the stream is synchronised; count[i] (host, n) tokens and rows of sentence i are valid
 * and FINAL: a row never changes afterwards; done[i] (host, n) is 1 when count[i] is the sentence's n_out (a sentence with
 * max_new == 0 is done with count 0 from the start); *finished is 1 when no sentence is live or waiting.  stats (host, 2 ints,
 * or NULL): as mi_gpt_generate_queue, so far.  A call after *finished does nothing and reports the same.
 *
 * mi_gpt_queue_end: closes the session; it may come before *finished (the rest is abandoned) and the handle is usable
 * afterwards.  mi_gpt_destroy with an open session is fine.
 *
 * While a session is open every other entry on the handle that would touch the slots returns MI_ESTATE: mi_gpt_step,
 * mi_gpt_generate*, mi_gpt_kv_write, mi_gpt_reset, mi_gpt_bench_pick and a second mi_gpt_queue_begin; advance / end without a
 * session return MI_ESTATE too; all of this covers mi_gpt_generate_queue_beam and mi_gpt_queue_begin_beam as well.  Beam search
 * goes through a session opened by mi_gpt_queue_begin_beam (below): hypothesis 0's rows are gathered along its ancestors when its
 * sentence ends, so no row of a sentence is final before that, and count[i] stays 0 until sentence i is retired.             */
int         mi_gpt_queue_begin(mi_gpt* h, int n, const float* prompts, const int32_t* prompt_rows, const int32_t* max_new,
                               const int32_t* stop_ids, int n_stop, float repeat_value, int penalty_range, int32_t* tokens,
                               float* hidden, int cap, int mem, const float* temperature, const int32_t* top_k, const float* top_p,
                               const uint64_t* seeds);
int         mi_gpt_queue_advance(mi_gpt* h, int32_t* count /* host, n */, int32_t* done /* host, n */, int32_t* finished /* host, 1 */,
                                 int32_t* stats /* host, 2 ints, or NULL */);
int         mi_gpt_queue_end(mi_gpt* h);

/* ---- beam search through the sentence queue: a sentence runs as a group, B = num_beams hypotheses in B consecutive slots, and
 * the queue schedules groups where it schedules slots above.  The beam search is the one defined under "beam search" in every
 * respect (selection 0, selection n, the end rule, ties, no finished pool, no length penalty).
 *
 * mi_gpt_generate_queue_beam: arguments and validation of mi_gpt_generate_queue without the sampling arrays (beams and sampling
 * do not combine), plus mi_gpt_generate_beam's checks on num_beams: 1..8, at most mel_codes, at most max_batch.  All of it runs
 * before anything is launched: MI_EINVAL, with the handle still usable.  scores (n) or NULL follows `mem`.  Per sentence the
 * result is what mi_gpt_generate_beam gives for that sentence alone from a penalty vector of ones: hypothesis 0's tokens, its
 * last_hidden_state rows along its own path, and its score.  The decode steps are the same launches; the prompt pass differs
 * from the one-by-one pass in GEMM tiling only, as for the greedy queue; there is no repeat_penality argument and no write-back,
 * for the reason given there.  num_beams == 1 gives the tokens of mi_gpt_generate_queue.
 *
 * Policy (mi355tts.indextts.queue_schedule(..., beams=B), i.e. with slots = max_batch / B, is its host model).  G = min(max_batch
 * / B, n) groups; group g is slots gB .. gB + B - 1; slots beyond G * B are never run and the decode step runs over G * B rows.
 * Steps 1-3 are the ones above with "slot" read as "group": admission in index order into the lowest free group, a pass ending
 * at the first sentence whose rows would push it past max_seq packed rows; retire, then refill before the next decode step; runs
 * of c = min(16, nearest limit of a live group) beam decode steps over the G groups.  A pass stores each prompt's keys and values
 * once, in its group's first slot, and selection 0 of all the groups it admitted is one launch.  Every group retiring in a round
 * leaves in one launch (tokens, rows and score, along the ancestor table) ahead of the pass that refills it.  stats: as above.
 *
 * mi_gpt_queue_begin_beam: the same arguments; it opens the kind of session mi_gpt_queue_advance / mi_gpt_queue_end drive, and
 * `scores` stays the caller's until mi_gpt_queue_end like tokens and hidden.  count[i] is 0 until sentence i is retired, then it
 * is its n_out with done[i] = 1: its tokens, rows and score all leave in that round.                                         */
int         mi_gpt_generate_queue_beam(mi_gpt* h, int n, const float* prompts, const int32_t* prompt_rows, const int32_t* max_new,
                                       const int32_t* stop_ids, int n_stop, float repeat_value, int penalty_range, int num_beams,
                                       int32_t* tokens, float* hidden, int cap, int32_t* n_out, float* scores /* (n) or NULL */,
                                       int mem, int32_t* stats /* host, 2 ints or NULL */);
int         mi_gpt_queue_begin_beam(mi_gpt* h, int n, const float* prompts, const int32_t* prompt_rows, const int32_t* max_new,
                                    const int32_t* stop_ids, int n_stop, float repeat_value, int penalty_range, int num_beams,
                                    int32_t* tokens, float* hidden, int cap, float* scores /* (n) or NULL */, int mem);

/* ---- pool mode through the sentence queue: the groups above running "beam search with a finished pool" (selections 1-9, ties,
 * Philox counters, K = (n_stop + 1) * B exactly as defined there), deterministic or sampled.  This is upstream IndexTTS' own
 * decode configuration (num_beams = 3, do_sample, top_k = 30, top_p = 0.8, length_penalty = 0) with slot refill, packed prompt
 * passes, sessions and streaming.
 *
 * mi_gpt_generate_queue_beam_pool: the arguments of mi_gpt_generate_queue_beam, then length_penalty, early_stopping and four HOST
 * arrays of n sampling parameters (all four NULL: deterministic), as mi_gpt_generate_beam_pool takes them.  Validation is the
 * union of the two entries': lengths per sentence; num_beams 1..8, at most mel_codes, at most max_batch; K <= 64 and <= mel_codes;
 * length_penalty finite; early_stopping 0 or 1; valid sampling records, all four arrays or none; top_k 0 or >= K; at most 16384
 * mel codes with sampling.  All of it runs before anything is launched: MI_EINVAL, the handle still usable and no session open.
 * There is no repeat_penality argument: every sentence starts from ones, as in the other queue entries.
 *   Contract: per sentence the result (tokens, rows, n_out, score) is what mi_gpt_generate_beam_pool gives for that sentence
 *   alone from a penalty vector of ones.  The decode steps are the same launches; the prompt pass differs from the one-by-one
 *   pass in GEMM tiling only.  A sampled sentence's result depends on its seed alone: not on its group, its pass or n.
 * Policy: the one above, a unit being a group.  max_new bounds the SELECTIONS a sentence runs (the prompt pass's selection 0
 * included), which is what the schedule counts; the length a sentence returns is that of pool entry 0 and is usually smaller.
 * So stats, and mi_gpt_queue_schedule(..., beams = B) as their host model, take lengths[i] = the selections sentence i ran, not
 * its returned length.  A pass that admits k groups makes each group's pool empty (in stream order behind the retirement of the
 * tenant before) and runs selection 0 of all k in one launch; every group retiring in a round leaves in one launch along its
 * frozen list, ahead of the pass that refills it.  A sentence with max_new == 0 takes no group: n_out 0, score 0.
 *
 * mi_gpt_queue_begin_beam_pool: the same arguments without n_out and stats; the session mi_gpt_queue_advance / mi_gpt_queue_end
 * drive, exactly as mi_gpt_queue_begin_beam's: count[i] is 0 until sentence i is retired, then its n_out with done[i] = 1, its
 * tokens, rows and score leaving in that round.  While it is open the MI_ESTATE rules above hold (mi_gpt_generate_beam_pool and
 * these two entries included).                                                                                              */
int         mi_gpt_generate_queue_beam_pool(mi_gpt* h, int n, const float* prompts, const int32_t* prompt_rows,
                                            const int32_t* max_new, const int32_t* stop_ids, int n_stop, float repeat_value,
                                            int penalty_range, int num_beams, float length_penalty, int early_stopping,
                                            const float* temperature, const int32_t* top_k, const float* top_p,
                                            const uint64_t* seeds /* host, n; all four or none */, int32_t* tokens, float* hidden,
                                            int cap, int32_t* n_out, float* scores /* (n) or NULL */, int mem,
                                            int32_t* stats /* host, 2 ints or NULL */);
int         mi_gpt_queue_begin_beam_pool(mi_gpt* h, int n, const float* prompts, const int32_t* prompt_rows, const int32_t* max_new,
                                         const int32_t* stop_ids, int n_stop, float repeat_value, int penalty_range, int num_beams,
                                         float length_penalty, int early_stopping, const float* temperature, const int32_t* top_k,
                                         const float* top_p, const uint64_t* seeds, int32_t* tokens, float* hidden, int cap,
                                         float* scores /* (n) or NULL */, int mem);

/* Tests and tools, no handle, no GPU: the schedule the policy above gives n sentences that will produce lengths[i] tokens each
 * (host arrays of n; 1 <= lengths[i] <= max_new[i], or 0 where max_new[i] is 0) on a handle of `slots` slots and max_seq packed
 * rows, in units of `beams` slots (1: no beam search).  The library's own policy object is driven as the engine drives it: the
 * prompt pass gives token 0 and a unit is done when its sentence holds lengths[i] tokens.  *steps / *n_passes: what stats would
 * report; pass_of[i]: the pass that admitted sentence i, counted from 0; unit_of[i]: the slot (beams > 1: the group) it was
 * admitted into; both -1 where max_new[i] is 0.  Inside a pass sentences are in index order, so this is the whole of
 * mi355tts.indextts.queue_schedule's result, and its argument errors are the ones reported here (MI_EINVAL).             */
int         mi_gpt_queue_schedule(int n, const int32_t* prompt_rows, const int32_t* max_new, const int32_t* lengths, int slots,
                                  int max_seq, int beams, int32_t* steps, int32_t* n_passes, int32_t* pass_of /* n */,
                                  int32_t* unit_of /* n */);

/* tuning hook: microseconds per launch (HIP events around `iters` launches) of the decode step's token-choosing kernel over nb
 * slots, on the logits the handle's last step left: the greedy kernel when temperature is NULL, else the sampler with these
 * host arrays of nb parameters.  The slots are marked done for the measurement: no token is stored and no state moves.    */
int         mi_gpt_bench_pick(mi_gpt* h, int nb, int iters, const float* temperature, const int32_t* top_k, const float* top_p,
                              double* us);

/* tuning hook: time `iters` launches of the implicit-GEMM conv kernel on random device data (no host copies);
 * returns average milliseconds per launch in *ms.  x (B,T,Cin), w (N, taps*Cin), out (B,T,N), "same" padding. */
int         mi_bench_conv_gemm(int dtype, int B, int T, int Cin, int N, int taps, int dil, int with_res, int iters,
                               double* ms);

/* host only, no device needed: the launch plan of that same convolution (the arguments of mi_bench_conv_gemm, at the process's
 * options) on a device of `cus` compute units.  *n_launches = 1, or 2 when the rows are split; plans[launch][MI_GEMM_PLAN_INTS] =
 * kind, Tm, Tn, RT, RC, lds_epi, use_buf, grid x, y, z.  kind counts from 1 in this order: direct 256x32, direct 128x64, direct
 * 128x128, DMA 64x64, DMA 64x64 with fp16 pairs, DMA 128 two-buffer, DMA 128 four-stage ring, ph8, x3p, x3, stream-K, dma3 at
 * 192, at 256, at 128.  (The grouped-convolution kernels are tried before the plan and decide for themselves.)            */
#define MI_GEMM_PLAN_INTS 10
int         mi_conv_gemm_plan(int dtype, int B, int T, int Cin, int N, int taps, int dil, int with_res, int cus,
                              int32_t* plans /* [2][MI_GEMM_PLAN_INTS] */, int* n_launches);

/* ---- IndexTTS graph A: prompt audio -> conditioning (cond.hip) -----------------------------------------------------------
 * Replaces ort_session_A of IndexTTS/Inference_IndexTTS_ONNX.py:700-712 (graph definition: IndexTTS_A,
 * IndexTTS/Export_IndexTTS.py:74-200): mel front end (0.1 s constant noise pad + 'constant'-padded STFT + HTK mel + log) ->
 * Conformer conditioning encoder (rel-pos attention with rel_shift) -> Perceiver resampler => conds_latent (latents, model_dim),
 * the prompt of the acoustic GPT (graph D's first input); ECAPA-TDNN speaker encoder + the 1x1 conditioning convolutions =>
 * conds = [bigvgan_cond_layer_speaker_embedding (voc_initial) | save_bigvgan_conds_0 | ... | _n-1] (mi_bigvgan_forward_latent
 * takes the same vectors with the speaker-embedding layer's LAST: IndexCond.split_conds / graph F's input order).  fp32 engine.  cfg: mi355tts.config.IndexCondConfig.to_int_array(); weights: the packed
 * blob of mi355tts.weights.pack_cond (export-time folds applied).  mel (optional, may be NULL): the (frames, n_mels) log-mel. */
int64_t     mi_indextts_cond_param_count(const int32_t* cfg, int n_cfg);
mi_cond*    mi_indextts_cond_create(const int32_t* cfg, int n_cfg, const float* weights, int64_t n_weights, int device);
void        mi_indextts_cond_destroy(mi_cond* h);
int         mi_indextts_cond_run(mi_cond* h, const int16_t* audio, int64_t L, float* conds, float* conds_latent, float* mel,
                                 int mem);

/* Process-wide tuning / A-B switches (tools, tests), one table (csrc/options.h).  Precedence, for every key: the default, then the
 * environment variable of the key where it has one (the whole table is read ONCE, at the process's first call into the library),
 * then mi_set_option.  mi_get_option reports what the process runs with.  Out-of-range values: the "attn_*" keys,
 * "bigvgan_streams" (1..3) and "gemm_ph8_split_max" (1..4) clamp; "gemm_f32_planes" / "attn_f32_planes" take 2 or 3 and the call
 * fails otherwise (mi_last_error names the key, the value stays); on/off keys store value != 0; the rest store the value as given.
 * Thread safety: every entry point that DISPATCHES KERNELS (create / run / step /
 * generate / forward ...) holds the shared side of one reader-writer lock for its duration and mi_set_option the exclusive side — a
 * change waits for the calls in flight on other threads (under sustained concurrent inference that wait is unbounded: the lock
 * prefers readers; set options before serving) and is seen as a whole by the calls that start after it; it never alters the dispatch
 * of a call that is running.  mi_*_destroy, mi_last_error, mi_device_count and mi_version read no option and take no lock.
 *  The arithmetic of an fp32 F5 engine is NOT one of them any more: it is a
 * property of the engine (config int 21, F5Config.f32_arithmetic; mi_f5_info reports what runs) — the four arithmetic keys below
 * only set the default of engines created without one.
 *   arithmetic defaults: "gemm_f32_x3" (1: fp32 linear layers from 16-bit partial products, 0: native v_mfma_f32_32x32x2_f32),
 *     "gemm_f32_planes" (2: fp16 {hi, lo * 2^11} pairs, 22-bit operands, |a| <= 65504 — watched, see mi_f5_info; 3: three bf16
 *     planes, exact), "attn_f32_x3" (2: both attention products split, 1: q.k only, 0: native), "attn_f32_planes" (2 | 3);
 *     "gemm_f32_x3p" (0: the round-2 kernel gemm_x3.hip instead of the panel-plane kernel), "gemm_f32_n64_pairs" /
 *     "gemm_f32_gconv" (the position convolution on fp16 pairs / with each operand split once per workgroup),
 *     "gconv_two_taps" (0: re-split the position convolution's weights per launch instead of using the planes split at load),
 *     "gconv16" (0: the 16-bit engines' position convolution on the generic tile kernel instead of gconv16.hip)
 *   dispatch thresholds of the implicit-GEMM launcher: "gemm_big_tile_min", "gemm_n192_min", "gemm_mid_tile_min",
 *     "gemm_dma3_k_min", "gemm_use_dma3", "gemm_use_dma", "gemm_big_tiles", "gemm_n192", "gemm_f32_dma", "gemm_ring4",
 *     "gemm_ring4_max", "gemm_buf", "gemm_f32_small", "gemm_f32_small_max", "gemm_small16_max", "gemm_sk" (stream-K: 0 off, 1 fp32,
 *     2 also 16-bit), "gemm_sk_stages", "gemm_ph8", "gemm_ph8_min_tiles", "gemm_ph8_order", "gemm_ph8_split_max", "gemm_ph8_split_min_nk" (split tail, tests), "gemm_row_split",
 *     "gemm_x3p_grid" (XCD bands: 0 automatic, else 1 / 2 / 4 / 8 row bands), "gemm_x3p_noalign"
 *   attention: "attn_split" (small grids: 0 plain 128-query workgroups, 1 64-query workgroups with the keys split between wave
 *     pairs + key slices, 2 [default] fp32: 128-query workgroups + key slices, 16-bit as 1), "attn_kv_planes" (0: the fp32 kernel splits K / V itself), "attn_z_force" (key slices, tests),
 *     "attn_xcd_map" (1: a head's query tiles on one XCD; bit-identical either way),
 *     "attn_lpt" (1 [default]: the fp32 128-query kernel's key slices are uneven, longest first — attention.hip attn_pick_slices),
 *     "gemm_x3d" (1 [default]: fp32 linear layers on the exact-fit data-parallel kernel gemm_x3d.hip when the output divides into whole rounds
 *     of the CUs), "gemm_x3d_min_eff" (per cent of useful tile area from which it is taken, default 90)
 *   "gpt_mfma_min" (sentences from which mi_gpt_generate_batch runs its linears on MFMA; default 9)
 *   "bigvgan_streams" (default 3): the AMP blocks of a BigVGAN stage on side streams of the handle — 1: one stream; 2: only
 *     the stages whose AMP halves are separate AA and conv launches (C > 96); 3: every stage.  Bit-identical in all three.
 *   BigVGAN's anti-aliased activation kernels in 16-bit storage (A/B and test switches; every setting gives the same bits):
 *     "aa_tile" (elements per tile, rows x channels; default 8192), "aa_pipe" (0: one tile per workgroup instead of persistent
 *     workgroups with LDS-DMA), "aa_r" (16 | 8 outputs per work item of the pipelined kernel), "aaconv_lds_min" (bytes of LDS the
 *     fused AA + conv kernel asks for at least; 83968: one workgroup per CU instead of two)
 * Removed in round 4 (variants that lost their A/B, nothing used them): "gemm_sk_min_tiles", "gemm_sk_max_tiles", "gemm_sk_qkv32",
 * "gemm_f32_n64_dma", "gemm_n64_dma16", "attn_z_max", "attn_z16_max",
 * "aa_conv_deterministic".  Changing an option invalidates the hipGraphs captured by existing handles.   */
int         mi_set_option(const char* key, int64_t value);
/* The current value of a mi_set_option key into *value (no GPU needed).  Fails for an unknown key or a null pointer. */
int         mi_get_option(const char* key, int64_t* value);
/* PCI bus id of HIP device `device` ("0000:05:00.0") into buf: multi-rank launchers use it to check that every rank drives its
 * own GPU (mi355tts/shard.py assert_one_device_per_rank).  No reference counterpart (the reference is single-device).   */
int         mi_device_pci_bus_id(int device, char* buf, int cap);

/* ---- profiling hooks (bench.py roofline leg) -------------------------------------------------
 * family_mask: bit i enables family i (0 = off, -1 = all).  Every launch of an enabled kernel
 * family is bracketed by HIP events on the handle's own stream; mi_prof_get returns accumulated
 * milliseconds, launches and algorithmic bytes / flops since the last reset.
 * Families (bit): "conv_gemm"(0) "aa_act"(1) "conv_post"(2) "attn"(3) "norm"(4) "other"(5).    */
int         mi_prof_enable(int family_mask);
int         mi_prof_reset(void);
int         mi_prof_get(const char* family, double* ms, int64_t* launches, double* bytes, double* flops);
/* The same accumulators per kernel instantiation (name = the template instantiation rocprofv3 --kernel-trace lists, e.g.
 * "conv_gemm_dma_kernel<float, float, true, 2, 64>"; launches that do not name their kernel are filed under the family
 * name).  index in [0, mi_prof_kernel_count()).                                                                        */
int         mi_prof_kernel_count(void);
int         mi_prof_kernel_get(int index, char* name, int name_cap, char* family, int family_cap, double* ms,
                               int64_t* launches, double* bytes, double* flops);

#ifdef __cplusplus
}
#endif
#endif /* MI355TTS_H */
