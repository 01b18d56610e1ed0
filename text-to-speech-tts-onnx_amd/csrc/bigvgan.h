// bigvgan.h — BigVGAN-v2 engine object (see bigvgan.hip).
#pragma once
#include "common.h"

namespace mi {

struct BigVGANCfg {
    int num_mels = 0, c0 = 0, n_up = 0, n_kernels = 0, bias_final = 0, tanh_final = 1, logscale = 1, n_dil = 0;
    int pre_ln = 0, cond = 0;          // IndexTTS graph F: LayerNorm in front, speaker-conditioning biases
    int hop = 1;
    std::vector<int> rates, up_k, res_k;
    std::vector<std::vector<int>> dil;
};
BigVGANCfg parse_bigvgan_cfg(const int32_t* c, int n);
int64_t bigvgan_param_count(const BigVGANCfg& g);

struct ConvW { DevBuf w, b; std::vector<float> hb; DevBuf b_eff; };   // hb / b_eff: bias + per-call speaker conditioning
struct SnakeP { DevBuf alpha, inv_beta; };
struct AmpBlock { int k = 3; std::vector<ConvW> c1, c2; std::vector<SnakeP> acts; };
struct Stage { int cin = 0, cout = 0, u = 1, k = 2; ConvW up; std::vector<AmpBlock> blocks; };

struct BigVGAN {
    BigVGANCfg cfg;
    int dtype, device;
    hipStream_t stream = nullptr;
    int mel_pad = 0;
    ConvW pre;
    std::vector<Stage> stages;
    SnakeP post_act;
    DevBuf post_w;
    float post_bias = 0.f;
    // workspace
    int ws_B = 0, ws_F = 0;
    DevBuf bIN, bX, bT1, bT2, bP, bQ, d_mel, d_out_f32, d_out_i16;
    // the AMP blocks of a stage (one per resblock kernel size) only share their input X and the accumulation into IN: blocks
    // 1.. run on side streams with scratch buffers of their own (option "bigvgan_streams", bigvgan.hip body())
    static constexpr int MAX_SIDE = 3;
    hipStream_t side[MAX_SIDE] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_x = nullptr, ev_last[MAX_SIDE + 1] = {nullptr, nullptr, nullptr, nullptr};
    DevBuf sT1[MAX_SIDE], sT2[MAX_SIDE], sP[MAX_SIDE], sQ[MAX_SIDE];
    hipStream_t ls = nullptr;      // launch stream of conv / aa / aa_conv (null: `stream`)
    void ensure_side(int n);

    BigVGAN(const BigVGANCfg& g, const float* w, int64_t nw, int dt, int dev);
    ~BigVGAN();
    void ensure_workspace(int B, int F);
    void conv(const ConvW& cw, const void* x, void* out, int B, int T, int Cin, int Cout, int k, int dil,
              const void* res, float alpha, int accumulate);
    void aa(const SnakeP& sp, const void* x, void* y, int B, int T, int C, int post);
    void aa_conv(const SnakeP& sp, const ConvW& cw, const void* x, void* out, int B, int T, int C, int k, int dil,
                 const void* res, float alpha, int accumulate);
    int fused_max_c = 96;
    bool use_fused = true;     // MI355TTS_NO_FUSED_AA=1 selects the unfused AA + conv path (A/B and debugging)
    void run(const float* mel, int B, int F, float* out_f32, int16_t* out_i16, int mem);
    // ragged batches (padded slabs of Fmax frames, item b live in its first frames[b]): mel = the items' (num_mels, frames[b])
    // arrays concatenated; the waveforms (frames[b] * hop + 30 samples each) leave concatenated in the same order
    void run_ragged(const float* mel, int B, const int* frames, float* out_f32, int16_t* out_i16, long out_cap, int64_t* out_lens, int mem);
    // ... and graph F: latent = the items' (T_codes[b], num_mels) rows concatenated; item b speaks with voice voice_of[b] (host, B
    // ints in [0, n_voices)), conds = (n_voices, n_conds) rows in run_latent's layout (follows `mem`).  The seven speaker biases
    // become one device table of B rows (cond_bias_table_kernel) that conv_pre and the upsamplers index by item.
    void run_latent_voices(const float* latent, int B, const int* T_codes, int n_voices, const float* conds, long n_conds,
                           const int* voice_of, float* out_f32, int16_t* out_i16, long out_cap, int64_t* out_lens, int mem);
    // ... windows of one (latent_rows, num_mels) array instead of whole sentences: item b = rows [row0[b], row0[b] + rows[b]), no
    // rows dropped, head[b] / tail[b] halo frames whose samples are computed and not written (conv_post's windowed instantiation)
    void run_latent_windows(const float* latent, long latent_rows, int B, const int64_t* row0, const int64_t* rows, const int32_t* head,
                            const int32_t* tail, int n_voices, const float* conds, long n_conds, const int* voice_of, float* out_f32,
                            int16_t* out_i16, long out_cap, int64_t* out_lens, int mem);
    // what the two share once their arguments are checked (row0 / win null: sentences one after another, untrimmed tail)
    void latent_items(const float* latent, long rows, int B, const int* F, int Fmax, const long* row0, const long* win, long total,
                      int n_voices, const float* conds, long n_conds, const int* voice_of, float* out_f32, int16_t* out_i16,
                      int64_t* out_lens, int mem);
    // ... the one-voice form of run_latent_voices: n_voices = 1, voice_of = 0 ... 0
    void run_latent_ragged(const float* latent, int B, const int* T_codes, const float* conds, long n_conds, float* out_f32,
                           int16_t* out_i16, long out_cap, int64_t* out_lens, int mem);
    // IndexTTS graph F: latent (T_codes, num_mels) channels-last fp32, conds = [cond_0 .. cond_{n_up-1}, cond_pre] concatenated
    void run_latent(const float* latent, int T_codes, const float* conds, long n_conds, float* out_f32, int16_t* out_i16, int mem);
    // graph F's speaker conditioning: cond_ptrs = host vectors added per layer on the host (run_latent), or tab = the device table
    // of layer bias + conditioning, row b for item b, tab_stride floats apart (run_latent_voices); both null: the layers' own biases
    void body(const void* x0, int B, int F, const float* const* cond_ptrs, const float* tab, long tab_stride, float* out_f32,
              int16_t* out_i16, int mem);
    // lengths of the current ragged call (null: uniform): d_frames = F_b per item; every launch of body() gets the table with
    // the (mul, add) of its resolution; conv_post writes item b from sample d_out_offs[b] of the output (total samples)
    const int* ln = nullptr; int ln_mul = 1;
    DevBuf d_frames, d_in_offs, d_out_offs;
    DevBuf d_voice_of, d_conds, d_bias_tab;       // run_latent_voices: voice per item, the host caller's conditioning rows, the (B, total_cond) bias table
    const long* out_offs = nullptr; long out_total = 0;
    bool out_win = false;                         // d_out_offs holds conv_post's window table (3 values per item)
    // uploads (voice_of, when given, goes up with them); returns the output offsets.  row0: the items' first input rows instead of
    // running sums; win: the (first kept sample, kept count, output offset) table of a windowed call instead of the output offsets
    std::vector<long> ragged_tables(int B, const int* frames, long extra_rows, const int* voice_of = nullptr, const long* row0 = nullptr,
                                    const long* win = nullptr);
    long total_cond() const;
    DevBuf ln_w, ln_b, d_latent;
};

void unit_aa_activation1d(const float* x, int B, int C, int T, const float* alpha_log, const float* beta_log,
                          int logscale, int post, int dtype, float* y);
void unit_aa_conv1d(const float* x, int B, int C, int T, const float* alpha_log, const float* beta_log, int logscale,
                    const float* w, const float* bias, int k, int dil, const float* res, int dtype, int repeat, float* y);
void unit_conv1d(const float* x, int B, int Cin, int T, const float* w, const float* bias, int Cout, int k, int dil,
                 int padding, int groups, int dtype, float* y);
void unit_conv_transpose1d(const float* x, int B, int Cin, int T, const float* w, const float* bias, int Cout, int k,
                           int stride, int padding, int dtype, float* y);


// runtime.hip
const std::string& last_error();
void prof_enable(unsigned mask);
void prof_reset();
int prof_family(const char* name);
void prof_get(int fam, double* ms, int64_t* launches, double* bytes, double* flops);
int prof_kernel_count();
bool prof_kernel_get(int idx, std::string* name, int* fam, double* ms, int64_t* launches, double* bytes, double* flops);

}  // namespace mi
