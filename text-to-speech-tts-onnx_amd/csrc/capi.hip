// capi.hip — extern "C" boundary of libmi355tts.so (declarations: include/mi355tts.h).
#include "common.h"
#include "bigvgan.h"
#include "f5.h"
#include "gpt.h"
#include "gpt_queue.h"
#include "gpt_pool.h"
#include "cond.h"
#include <algorithm>
#include <memory>
#include <mutex>
#include <exception>

using namespace mi;

// calls on one handle are serialised (one HIP stream + one workspace per handle); different handles run concurrently
struct mi_bigvgan { BigVGAN* impl; std::mutex mu; };
struct mi_f5 { F5* impl; std::mutex mu; };
struct mi_gpt { Gpt* impl; std::mutex mu; std::unique_ptr<GptQueue> session; };     // session: open from mi_gpt_queue_begin to _end
struct mi_cond { Cond* impl; std::mutex mu; };

// Every C-ABI entry runs under the SHARED side of the option lock; mi_set_option takes the exclusive side.  The dispatch options
// stay process-wide (tools, A/B runs, tests), but a change can never land in the middle of a call on another thread: it waits for
// the calls in flight, and calls that start afterwards see the whole new table (the header's promise that
// different handles may be driven from different threads holds with mi_set_option in the picture).
template <typename F> static int guard(F&& f, bool exclusive = false) {
    try {
        options_init();           // the process's first C-ABI call reads the environment into the option table (options.h)
        std::shared_lock<std::shared_mutex> rd(option_lock(), std::defer_lock);
        std::unique_lock<std::shared_mutex> wr(option_lock(), std::defer_lock);
        if (exclusive) wr.lock(); else rd.lock();
        f();
        return MI_OK;
    } catch (const mi::Error& e) {
        set_last_error(e.what());
        return e.code;
    } catch (const std::bad_alloc&) {
        set_last_error("out of host memory");
        return MI_ENOMEM;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return MI_EINVAL;
    }
}

// Runs `body` (launches + a stream synchronisation).  fp16-pair engines: if a producer flagged an operand at the fp16 range limit
// (x3_split.h sat_publish) the results of the call are not fp32-equivalent — the engine switches itself to the exact three-plane
// bf16 split (permanently; mi_f5_info reports it) and the body runs again.  `body` must not have overwritten its inputs.
template <typename F> static void f5_run_checked(F5& e, F&& body) {
    body();
    if (e.dtype == MI_F32 && e.np == 2 && e.take_saturation()) {
        ++e.sat_events;
        e.set_arith(ARITH_BF16X3);
        ArithScope sc(e.arith);          // (the caller's scope still holds the pair override)
        body();
        (void)e.take_saturation();
    } else if (e.dtype == MI_F16 && e.fold_built && e.cfg.ln_fold != 0 && e.take_saturation()) {
        // f16 engine: the AdaLN fold's A operand (the unnormalised residual row o (1 + scale)) left the fp16 range — the row-norm
        // path's operand LN(x) (1 + scale) + shift is bounded by the norm: fold off for this engine, permanently, and run again
        ++e.sat_events;
        e.cfg.ln_fold = 0;
        e.drop_graphs();
        body();
        (void)e.take_saturation();
    }
}

extern "C" {

const char* mi_version(void) { return "mi355tts 0.1 (gfx950)"; }
const char* mi_last_error(void) { return last_error().c_str(); }

int mi_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int mi_init(int device) {
    return guard([&] {
        int n = 0;
        MI_HIP(hipGetDeviceCount(&n));
        MI_REQUIRE(device >= 0 && device < n, "mi_init: no such HIP device (libmi355tts needs an MI355X; there is no CPU fallback)");
        MI_HIP(hipSetDevice(device));
        hipDeviceProp_t prop;
        MI_HIP(hipGetDeviceProperties(&prop, device));
        MI_REQUIRE(std::strncmp(prop.gcnArchName, "gfx950", 6) == 0, "mi_init: device is not gfx950");
        MI_HIP(hipFree(nullptr));
    });
}

int64_t mi_bigvgan_param_count(const int32_t* cfg, int n_cfg) {
    int64_t n = -1;
    int rc = guard([&] { n = bigvgan_param_count(parse_bigvgan_cfg(cfg, n_cfg)); });
    return rc == MI_OK ? n : (int64_t)rc;
}

mi_bigvgan* mi_bigvgan_create(const int32_t* cfg, int n_cfg, const float* weights, int64_t n_weights, int dtype,
                              int device) {
    mi_bigvgan* h = nullptr;
    int rc = guard([&] {
        MI_REQUIRE(weights != nullptr, "mi_bigvgan_create: null weights");
        BigVGANCfg g = parse_bigvgan_cfg(cfg, n_cfg);
        BigVGAN* impl = new BigVGAN(g, weights, n_weights, dtype, device);
        h = new mi_bigvgan; h->impl = impl;
    });
    return rc == MI_OK ? h : nullptr;
}

// a device-resident blob whose re-layouts are host code (BigVGAN conv / GPT Conv1D transposes): read back once at load
static std::vector<float> read_back(const float* dev, int64_t n, int device) {
    MI_REQUIRE(n > 0, "create_mem: empty blob");
    MI_HIP(hipSetDevice(device));
    std::vector<float> h((size_t)n);
    MI_HIP(hipMemcpy(h.data(), dev, (size_t)n * 4, hipMemcpyDeviceToHost));
    return h;
}

mi_bigvgan* mi_bigvgan_create_mem(const int32_t* cfg, int n_cfg, const float* weights, int64_t n_weights, int dtype,
                                  int device, int mem) {
    if (mem == MI_HOST) return mi_bigvgan_create(cfg, n_cfg, weights, n_weights, dtype, device);
    mi_bigvgan* h = nullptr;
    int rc = guard([&] {
        MI_REQUIRE(weights != nullptr && mem == MI_DEVICE, "mi_bigvgan_create_mem: null weights / bad mem kind");
        BigVGANCfg g = parse_bigvgan_cfg(cfg, n_cfg);
        MI_REQUIRE(n_weights == bigvgan_param_count(g), "bigvgan: weight blob size does not match the config");
        std::vector<float> hw = read_back(weights, n_weights, device);
        BigVGAN* impl = new BigVGAN(g, hw.data(), n_weights, dtype, device);
        h = new mi_bigvgan; h->impl = impl;
    });
    return rc == MI_OK ? h : nullptr;
}

void mi_bigvgan_destroy(mi_bigvgan* h) {
    if (!h) return;
    delete h->impl;
    delete h;
}

int64_t mi_bigvgan_out_len(const mi_bigvgan* h, int frames) {
    if (!h || frames <= 0) return MI_EINVAL;
    return (int64_t)frames * h->impl->cfg.hop + 30;
}

int mi_bigvgan_forward(mi_bigvgan* h, const float* mel, int B, int frames, int16_t* out, int mem) {
    return guard([&] {
        MI_REQUIRE(h && h->impl, "mi_bigvgan_forward: null handle");
        std::lock_guard<std::mutex> lk_(h->mu);
        MI_REQUIRE(mem == MI_HOST || mem == MI_DEVICE, "mi_bigvgan_forward: bad mem kind");
        h->impl->run(mel, B, frames, nullptr, out, mem);
    });
}

int mi_bigvgan_forward_f32(mi_bigvgan* h, const float* mel, int B, int frames, float* out, int mem) {
    return guard([&] {
        MI_REQUIRE(h && h->impl, "mi_bigvgan_forward_f32: null handle");
        std::lock_guard<std::mutex> lk_(h->mu);
        MI_REQUIRE(mem == MI_HOST || mem == MI_DEVICE, "mi_bigvgan_forward_f32: bad mem kind");
        h->impl->run(mel, B, frames, out, nullptr, mem);
    });
}

int mi_bigvgan_forward_latent(mi_bigvgan* h, const float* latent, int T_codes, const float* conds, int64_t n_conds,
                              int16_t* out, float* out_f32, int mem) {
    return guard([&] {
        MI_REQUIRE(h && h->impl, "mi_bigvgan_forward_latent: null handle");
        std::lock_guard<std::mutex> lk_(h->mu);
        MI_REQUIRE(mem == MI_HOST || mem == MI_DEVICE, "mi_bigvgan_forward_latent: bad mem kind");
        h->impl->run_latent(latent, T_codes, conds, (long)n_conds, out_f32, out, mem);
    });
}

// ragged batches: lengths are host int64, checked before anything reaches the device (the handle stays usable)
static std::vector<int> bigvgan_lengths(const int64_t* lens, int B, int64_t lo, const char* what) {
    MI_REQUIRE(lens && B >= 1, what);
    std::vector<int> v(B);
    for (int b = 0; b < B; ++b) {
        MI_REQUIRE(lens[b] >= lo && lens[b] < (1L << 30), what);
        v[b] = (int)lens[b];
    }
    return v;
}

int mi_bigvgan_forward_ragged(mi_bigvgan* h, int B, const float* mel, const int64_t* frames, int16_t* out_i16, float* out_f32,
                              int64_t out_cap, int64_t* out_lens, int mem) {
    return guard([&] {
        MI_REQUIRE(h && h->impl, "mi_bigvgan_forward_ragged: null handle");
        std::lock_guard<std::mutex> lk_(h->mu);
        MI_REQUIRE(mem == MI_HOST || mem == MI_DEVICE, "mi_bigvgan_forward_ragged: bad mem kind");
        MI_REQUIRE(out_i16, "mi_bigvgan_forward_ragged: null out_i16");
        const std::vector<int> F = bigvgan_lengths(frames, B, 1, "mi_bigvgan_forward_ragged: B >= 1 items of >= 1 frames");
        h->impl->run_ragged(mel, B, F.data(), out_f32, out_i16, (long)out_cap, out_lens, mem);
    });
}

int mi_bigvgan_forward_latent_ragged(mi_bigvgan* h, int B, const float* latent, const int64_t* t_codes, const float* conds,
                                     int64_t n_conds, int16_t* out_i16, float* out_f32, int64_t out_cap, int64_t* out_lens, int mem) {
    return guard([&] {
        MI_REQUIRE(h && h->impl, "mi_bigvgan_forward_latent_ragged: null handle");
        std::lock_guard<std::mutex> lk_(h->mu);
        MI_REQUIRE(mem == MI_HOST || mem == MI_DEVICE, "mi_bigvgan_forward_latent_ragged: bad mem kind");
        MI_REQUIRE(out_i16, "mi_bigvgan_forward_latent_ragged: null out_i16");
        const std::vector<int> T = bigvgan_lengths(t_codes, B, 3, "mi_bigvgan_forward_latent_ragged: B >= 1 items of >= 3 latent rows");
        h->impl->run_latent_ragged(latent, B, T.data(), conds, (long)n_conds, out_f32, out_i16, (long)out_cap, out_lens, mem);
    });
}

int mi_bigvgan_forward_latent_voices(mi_bigvgan* h, int B, const float* latent, const int64_t* t_codes, int n_voices, const float* conds,
                                     int64_t n_conds, const int32_t* voice_of, int16_t* out_i16, float* out_f32, int64_t out_cap,
                                     int64_t* out_lens, int mem) {
    return guard([&] {
        MI_REQUIRE(h && h->impl, "mi_bigvgan_forward_latent_voices: null handle");
        std::lock_guard<std::mutex> lk_(h->mu);
        MI_REQUIRE(mem == MI_HOST || mem == MI_DEVICE, "mi_bigvgan_forward_latent_voices: bad mem kind");
        MI_REQUIRE(out_i16, "mi_bigvgan_forward_latent_voices: null out_i16");
        MI_REQUIRE(voice_of, "mi_bigvgan_forward_latent_voices: null voice_of");
        const std::vector<int> T = bigvgan_lengths(t_codes, B, 3, "mi_bigvgan_forward_latent_voices: B >= 1 items of >= 3 latent rows");
        // voice indices and counts are checked by the engine before anything reaches the device (the handle stays usable)
        h->impl->run_latent_voices(latent, B, T.data(), n_voices, conds, (long)n_conds, (const int*)voice_of, out_f32, out_i16,
                                   (long)out_cap, out_lens, mem);
    });
}

int mi_bigvgan_forward_latent_windows(mi_bigvgan* h, int B, const float* latent, int64_t latent_rows, const int64_t* row0,
                                      const int64_t* rows, const int32_t* head, const int32_t* tail, int n_voices, const float* conds,
                                      int64_t n_conds, const int32_t* voice_of, int16_t* out_i16, float* out_f32, int64_t out_cap,
                                      int64_t* out_lens, int mem) {
    return guard([&] {
        MI_REQUIRE(h && h->impl, "mi_bigvgan_forward_latent_windows: null handle");
        std::lock_guard<std::mutex> lk_(h->mu);
        MI_REQUIRE(mem == MI_HOST || mem == MI_DEVICE, "mi_bigvgan_forward_latent_windows: bad mem kind");
        MI_REQUIRE(out_i16, "mi_bigvgan_forward_latent_windows: null out_i16");
        MI_REQUIRE(B >= 1 && latent_rows >= 1 && latent_rows < (1L << 40), "mi_bigvgan_forward_latent_windows: B >= 1 windows of >= 1 latent rows");
        // windows, voices and counts are checked by the engine before anything reaches the device (the handle stays usable)
        h->impl->run_latent_windows(latent, (long)latent_rows, B, row0, rows, head, tail, n_voices, conds, (long)n_conds,
                                    (const int*)voice_of, out_f32, out_i16, (long)out_cap, out_lens, mem);
    });
}

int mi_aa_activation1d(const float* x, int B, int C, int T, const float* alpha_log, const float* beta_log,
                       int logscale, int post, int dtype, float* y) {
    return guard([&] {
        MI_REQUIRE(x && y && alpha_log && beta_log && B > 0 && C > 0 && T > 0, "mi_aa_activation1d: bad arguments");
        unit_aa_activation1d(x, B, C, T, alpha_log, beta_log, logscale, post, dtype, y);
    });
}

int mi_aa_conv1d(const float* x, int B, int C, int T, const float* alpha_log, const float* beta_log, int logscale,
                 const float* w, const float* bias, int k, int dilation, const float* res, int dtype, float* y) {
    return guard([&] {
        MI_REQUIRE(x && y && w && bias && alpha_log && beta_log && B > 0 && C > 0 && T > 0 && k > 0 && (k & 1) && dilation > 0,
                   "mi_aa_conv1d: bad arguments");
        unit_aa_conv1d(x, B, C, T, alpha_log, beta_log, logscale, w, bias, k, dilation, res, dtype, 1, y);
    });
}

int mi_conv1d(const float* x, int B, int Cin, int T, const float* w, const float* bias, int Cout, int k, int dilation,
              int padding, int groups, int dtype, float* y) {
    return guard([&] {
        MI_REQUIRE(x && w && y && B > 0 && Cin > 0 && Cout > 0 && T > 0 && k > 0 && dilation > 0 && groups > 0 && padding >= 0,
                   "mi_conv1d: bad arguments");
        unit_conv1d(x, B, Cin, T, w, bias, Cout, k, dilation, padding, groups, dtype, y);
    });
}

int mi_conv_transpose1d(const float* x, int B, int Cin, int T, const float* w, const float* bias, int Cout, int k,
                        int stride, int padding, int dtype, float* y) {
    return guard([&] {
        MI_REQUIRE(x && w && y && B > 0 && Cin > 0 && Cout > 0 && T > 0, "mi_conv_transpose1d: bad arguments");
        unit_conv_transpose1d(x, B, Cin, T, w, bias, Cout, k, stride, padding, dtype, y);
    });
}

// ---------------------------------------------------------------------------------------------------
// F5-TTS
// ---------------------------------------------------------------------------------------------------
int64_t mi_f5_param_count(const int32_t* cfg_i, int n_i, const float* cfg_f, int n_f) {
    int64_t n = -1;
    int rc = guard([&] { n = f5_param_count(parse_f5_cfg(cfg_i, n_i, cfg_f, n_f)); });
    return rc == MI_OK ? n : (int64_t)rc;
}

mi_f5* mi_f5_create(const int32_t* cfg_i, int n_i, const float* cfg_f, int n_f, const float* weights, int64_t n_weights,
                    int dtype, int device) {
    mi_f5* h = nullptr;
    int rc = guard([&] {
        MI_REQUIRE(weights != nullptr, "mi_f5_create: null weights");
        F5Cfg c = parse_f5_cfg(cfg_i, n_i, cfg_f, n_f);
        F5* impl = new F5(c, weights, n_weights, dtype, device);
        h = new mi_f5; h->impl = impl;
    });
    return rc == MI_OK ? h : nullptr;
}

mi_f5* mi_f5_create_mem(const int32_t* cfg_i, int n_i, const float* cfg_f, int n_f, const float* weights, int64_t n_weights,
                        int dtype, int device, int mem) {
    mi_f5* h = nullptr;
    int rc = guard([&] {
        MI_REQUIRE(weights != nullptr && (mem == MI_HOST || mem == MI_DEVICE), "mi_f5_create_mem: null weights / bad mem kind");
        F5Cfg c = parse_f5_cfg(cfg_i, n_i, cfg_f, n_f);
        F5* impl = new F5(c, weights, n_weights, dtype, device, mem);
        h = new mi_f5; h->impl = impl;
    });
    return rc == MI_OK ? h : nullptr;
}

void mi_f5_destroy(mi_f5* h) {
    if (!h) return;
    delete h->impl;
    delete h;
}

// runs F5::recover() when the call leaves by an exception (while the handle lock is still held)
struct F5Recover {
    F5* e; int n;
    explicit F5Recover(F5* e_) : e(e_), n(std::uncaught_exceptions()) {}
    ~F5Recover() { if (std::uncaught_exceptions() > n) e->recover(); }
};
#define F5_CHECK(h, mem, name)                                                     \
    MI_REQUIRE((h) && (h)->impl, name ": null handle");                            \
    std::lock_guard<std::mutex> lk_((h)->mu);                                      \
    F5Recover rec_((h)->impl);                                                     \
    ArithScope arith_((h)->impl->arith);                                           \
    MI_REQUIRE((mem) == MI_HOST || (mem) == MI_DEVICE, name ": bad mem kind")

int mi_f5_tables(mi_f5* h, float* time_expand, float* delta_t) {
    return guard([&] {
        MI_REQUIRE(h && h->impl, "mi_f5_tables: null handle");
        std::lock_guard<std::mutex> lk_(h->mu);
        F5& e = *h->impl;
        if (time_expand) std::memcpy(time_expand, e.h_time_expand.data(), e.h_time_expand.size() * 4);
        if (delta_t) std::memcpy(delta_t, e.h_delta.data(), e.h_delta.size() * 4);
    });
}

int64_t mi_f5_info(mi_f5* h, const char* key) {
    int64_t v = -1;
    int rc = guard([&] {
        MI_REQUIRE(h && h->impl && key, "mi_f5_info: null handle / key");
        std::lock_guard<std::mutex> lk_(h->mu);
        F5& e = *h->impl;
        ArithScope as(e.arith);
        const std::string k(key);
        if (k == "f32_arithmetic") v = e.dtype != MI_F32 ? -1 : !gemm_x3_enabled() ? ARITH_NATIVE : (gemm_x3p_enabled() ? e.np : ARITH_BF16X3);
        else if (k == "saturation_events") v = e.sat_events;
        else if (k == "adaln_fold") v = (e.fold_built && e.cfg.ln_fold != 0) ? 1 : 0;
        else if (k == "attn_v_rows") v = attention_kv_layout(0, e.dtype, true).v_rows;       // of an evaluation whose QKV epilogue pre-splits K / V
        else MI_REQUIRE(false, "mi_f5_info: unknown key");
    });
    return rc == MI_OK ? v : (int64_t)rc;
}

int mi_f5_preprocess(mi_f5* h, const int16_t* audio, int64_t L, const int32_t* text_ids, int64_t T, int64_t max_duration,
                     const float* noise_in, uint64_t seed, float* noise, float* rope_cos, float* rope_sin,
                     float* cat_mel_text, float* cat_mel_text_drop, int64_t* ref_signal_len, int mem) {
    return guard([&] {
        F5_CHECK(h, mem, "mi_f5_preprocess");
        F5& e = *h->impl;
        MI_REQUIRE(max_duration > 0 && max_duration <= e.cfg.max_len && T >= 0 && T < (1 << 20) && L > 0 && L < (1L << 31),
                   "mi_f5_preprocess: sizes");
        const int N = (int)max_duration;
        const int R = e.preprocess(1, audio, L, text_ids, (int)T, N, noise_in, seed, mem);
        hipStream_t s = e.stream;
        const size_t cd = e.cfg.cond_dim(), D = e.cfg.dim_head;
        copy_out(noise, e.d_noise.p, (size_t)N * e.cfg.mel * 4, mem, s);
        copy_out(rope_cos, e.rope_cos.p, (size_t)N * D * 4, mem, s);
        copy_out(rope_sin, e.rope_sin.p, (size_t)N * D * 4, mem, s);
        copy_out(cat_mel_text, e.d_cmt.p, (size_t)N * cd * 4, mem, s);
        copy_out(cat_mel_text_drop, e.d_cmtd.p, (size_t)N * cd * 4, mem, s);
        MI_HIP(hipStreamSynchronize(s));
        e.finish_call();
        if (ref_signal_len) *ref_signal_len = R;
    });
}

int mi_f5_transformer_step(mi_f5* h, float* noise, const float* cmt, const float* cmtd, int U, int64_t N,
                           int32_t* time_step, int fuse, int mem) {
    return guard([&] {
        F5_CHECK(h, mem, "mi_f5_transformer_step");
        MI_REQUIRE(noise && cmt && cmtd && time_step && fuse >= 1 && U >= 1 && N > 0, "mi_f5_transformer_step: bad arguments");
        F5& e = *h->impl;
        f5_run_checked(e, [&] {
            e.load_cond(noise, cmt, cmtd, U, (int)N, mem);
            e.build_cat_cond(U, (int)N);
            e.steps(U, (int)N, *time_step, fuse);
            MI_HIP(hipStreamSynchronize(e.stream));
        });
        copy_out(noise, e.d_noise.p, (size_t)U * N * e.cfg.mel * 4, mem, e.stream);
        MI_HIP(hipStreamSynchronize(e.stream));
        e.finish_call();
        *time_step += fuse;
    });
}

int mi_f5_sample(mi_f5* h, float* noise, const float* cmt, const float* cmtd, int U, int64_t N, int k0, int n_steps, int mem) {
    return guard([&] {
        F5_CHECK(h, mem, "mi_f5_sample");
        MI_REQUIRE(noise && cmt && cmtd && U >= 1 && N > 0, "mi_f5_sample: bad arguments");
        F5& e = *h->impl;
        f5_run_checked(e, [&] {
            e.load_cond(noise, cmt, cmtd, U, (int)N, mem);
            e.build_cat_cond(U, (int)N);
            e.steps(U, (int)N, k0, n_steps);
            MI_HIP(hipStreamSynchronize(e.stream));
        });
        copy_out(noise, e.d_noise.p, (size_t)U * N * e.cfg.mel * 4, mem, e.stream);
        MI_HIP(hipStreamSynchronize(e.stream));
        e.finish_call();
    });
}

int mi_f5_dit_eval(mi_f5* h, const float* noise, const float* cmt, const float* cmtd, int U, int64_t N, int k, float* pred, int mem) {
    return guard([&] {
        F5_CHECK(h, mem, "mi_f5_dit_eval");
        MI_REQUIRE(noise && cmt && cmtd && pred && U >= 1 && N > 0, "mi_f5_dit_eval: bad arguments");
        F5& e = *h->impl;
        f5_run_checked(e, [&] {
            e.load_cond(noise, cmt, cmtd, U, (int)N, mem);
            e.build_cat_cond(U, (int)N);
            e.dit_eval(U, (int)N, k);
            MI_HIP(hipStreamSynchronize(e.stream));
        });
        copy_out(pred, e.pred_rows(U, (int)N), (size_t)2 * U * N * e.cfg.mel * 4, mem, e.stream);
        MI_HIP(hipStreamSynchronize(e.stream));
        e.finish_call();
    });
}

int mi_f5_decode(mi_f5* h, const float* denoised, int U, int64_t N, int64_t ref_signal_len, int16_t* out, float* out_f32,
                 int64_t* out_len, int mem) {
    return guard([&] {
        F5_CHECK(h, mem, "mi_f5_decode");
        MI_REQUIRE(denoised && (out || out_f32) && U >= 1 && N > 0 && ref_signal_len >= 0 && ref_signal_len < N,
                   "mi_f5_decode: bad arguments");
        F5& e = *h->impl;
        e.load_cond(denoised, nullptr, nullptr, U, (int)N, mem);
        const long len = e.decode(e.d_noise.as<float>(), U, (int)N, (int)ref_signal_len, out_f32 ? e.v_outf.as<float>() : nullptr,
                                  out ? e.v_outi.as<int16_t>() : nullptr);
        copy_out(out, e.v_outi.p, (size_t)U * len * 2, mem, e.stream);
        copy_out(out_f32, e.v_outf.p, (size_t)U * len * 4, mem, e.stream);
        MI_HIP(hipStreamSynchronize(e.stream));
        e.finish_call();
        if (out_len) *out_len = len;
    });
}

int mi_f5_synthesize(mi_f5* h, int U, const int16_t* audio, int64_t L, const int32_t* text_ids, int64_t T,
                     int64_t max_duration, const float* noise_in, uint64_t seed, int16_t* out, int64_t* out_len, int mem) {
    return guard([&] {
        F5_CHECK(h, mem, "mi_f5_synthesize");
        MI_REQUIRE(audio && text_ids && out && U >= 1 && max_duration > 0, "mi_f5_synthesize: bad arguments");
        F5& e = *h->impl;
        const int N = (int)max_duration;
        long len = 0;
        f5_run_checked(e, [&] {
            const int R = e.preprocess(U, audio, L, text_ids, (int)T, N, noise_in, seed, mem);
            e.build_cat_cond(U, N);
            e.steps(U, N, 0, e.cfg.nfe - 1);
            len = e.decode(e.d_noise.as<float>(), U, N, R, nullptr, e.v_outi.as<int16_t>());
            copy_out(out, e.v_outi.p, (size_t)U * len * 2, mem, e.stream);
            MI_HIP(hipStreamSynchronize(e.stream));
        });
        e.finish_call();
        if (out_len) *out_len = len;
    });
}

// A -> loop, and the generated frames handed on as a mel for a vocoder engine: (U, 100, N - R) fp32, channels first — the
// `mel_features` layout of mi_bigvgan_forward (BigVGAN-v2 24khz_100band_256x shares F5's 100 bands / hop 256 / 24 kHz; the
// reference's bigvgan-type front end is modules.py:30-72).  *n_frames receives N - R.
int mi_f5_synthesize_mel(mi_f5* h, int U, const int16_t* audio, int64_t L, const int32_t* text_ids, int64_t T,
                         int64_t max_duration, const float* noise_in, uint64_t seed, float* mel_out, int64_t* n_frames, int mem) {
    return guard([&] {
        F5_CHECK(h, mem, "mi_f5_synthesize_mel");
        MI_REQUIRE(audio && text_ids && mel_out && U >= 1 && max_duration > 0, "mi_f5_synthesize_mel: bad arguments");
        F5& e = *h->impl;
        const int N = (int)max_duration;
        int F = 0;
        f5_run_checked(e, [&] {
            const int R = e.preprocess(U, audio, L, text_ids, (int)T, N, noise_in, seed, mem);
            const int mel = e.cfg.mel;
            F = N - R;
            MI_REQUIRE(F >= 1, "mi_f5_synthesize_mel: max_duration leaves no generated frames");
            e.build_cat_cond(U, N);
            e.steps(U, N, 0, e.cfg.nfe - 1);
            float* dst = mel_out;
            if (mem == MI_HOST) { e.v_outf.ensure((size_t)U * mel * F * 4); dst = e.v_outf.as<float>(); }
            for (int u = 0; u < U; ++u)
                launch_nlc_to_ncl(e.d_noise.as<float>() + ((size_t)u * N + R) * mel, dst + (size_t)u * mel * F, 1, mel, F, MI_F32, e.stream);
            if (mem == MI_HOST) copy_out(mel_out, dst, (size_t)U * mel * F * 4, mem, e.stream);
            MI_HIP(hipStreamSynchronize(e.stream));
        });
        e.finish_call();
        if (n_frames) *n_frames = F;
    });
}

// ragged batches (F5::dit_eval with lengths): lengths are host int64, checked before anything reaches the device
static std::vector<int> f5_lengths(const int64_t* lens, int U, int64_t lo, int64_t hi, const char* what) {
    MI_REQUIRE(lens && U >= 1, what);
    std::vector<int> v(U);
    for (int u = 0; u < U; ++u) {
        MI_REQUIRE(lens[u] >= lo && lens[u] <= hi, what);
        v[u] = (int)lens[u];
    }
    return v;
}

// The host plan of a ragged batch (mi_f5_synthesize_ragged / mi_f5_synthesize_mel_ragged: the same inputs and checks): lengths,
// prompt frames R_u, text ids, all checked before anything reaches the device.  `name` prefixes the messages.
struct F5RaggedPlan { std::vector<int> Ns, Ts, Rs; std::vector<long> Ls; int Nmax = 0; };
static F5RaggedPlan f5_ragged_plan(F5& e, int U, const int64_t* audio_lens, const int32_t* text_ids, const int64_t* text_lens,
                                   const int64_t* max_durations, int mem, const std::string& name) {
    const F5Cfg& c = e.cfg;
    F5RaggedPlan pl;
    pl.Ns = f5_lengths(max_durations, U, 1, c.max_len, (name + ": max_durations must be in [1, max_signal_length]").c_str());
    pl.Ts = f5_lengths(text_lens, U, 0, 1 << 20, (name + ": bad text length").c_str());
    pl.Ls.resize(U); pl.Rs.resize(U);
    const int mel_pad = c.mel_type == 1 ? (c.n_fft - c.hop) / 2 : c.n_fft / 2;
    int64_t ids = 0;
    for (int u = 0; u < U; ++u) {
        MI_REQUIRE(audio_lens && audio_lens[u] >= c.n_fft / 2 + 1 && audio_lens[u] > mel_pad && audio_lens[u] + 2 * mel_pad >= c.n_fft &&
                   audio_lens[u] < (1L << 31), name + ": audio shorter than one STFT frame");
        pl.Ls[u] = (long)audio_lens[u];
        pl.Rs[u] = e.ref_frames(pl.Ls[u]);
        MI_REQUIRE(pl.Ns[u] >= pl.Rs[u] + 1 && pl.Ns[u] >= pl.Ts[u], name + ": max_duration must exceed the prompt's frames and cover the text");
        ids += pl.Ts[u];
    }
    if (mem == MI_HOST)
        for (int64_t i = 0; i < ids; ++i)
            MI_REQUIRE((int64_t)text_ids[i] + 1 >= 0 && (int64_t)text_ids[i] + 1 <= c.vocab, name + ": text id out of range");
    pl.Nmax = *std::max_element(pl.Ns.begin(), pl.Ns.end());
    return pl;
}

// ... and its front end + sampling loop (inside f5_run_checked): the U slabs of d_noise hold the final latents afterwards
static void f5_ragged_loop(F5& e, int U, const int16_t* audio, const int32_t* text_ids, const float* noise_in, uint64_t seed, int mem,
                           F5RaggedPlan& pl) {
    e.preprocess_ragged(U, audio, pl.Ls.data(), text_ids, pl.Ts.data(), pl.Ns.data(), pl.Nmax, noise_in, seed, mem, pl.Rs.data());
    const int* lens = e.set_lengths(U, pl.Ns.data());
    e.build_cat_cond(U, pl.Nmax);
    e.steps(U, pl.Nmax, 0, e.cfg.nfe - 1, lens);
}

int mi_f5_synthesize_ragged(mi_f5* h, int U, const int16_t* audio, const int64_t* audio_lens, const int32_t* text_ids,
                            const int64_t* text_lens, const int64_t* max_durations, const float* noise_in, uint64_t seed, int16_t* out,
                            int64_t out_cap, int64_t* out_lens, int mem) {
    return guard([&] {
        F5_CHECK(h, mem, "mi_f5_synthesize_ragged");
        MI_REQUIRE(audio && text_ids && out && out_lens && U >= 1, "mi_f5_synthesize_ragged: bad arguments");
        F5& e = *h->impl;
        const F5Cfg& c = e.cfg;
        F5RaggedPlan pl = f5_ragged_plan(e, U, audio_lens, text_ids, text_lens, max_durations, mem, "mi_f5_synthesize_ragged");
        int64_t total = 0;
        for (int u = 0; u < U; ++u) total += (int64_t)(pl.Ns[u] - pl.Rs[u] - 1) * c.hop;
        MI_REQUIRE(total <= out_cap, "mi_f5_synthesize_ragged: out_cap is smaller than the sum of the waveform lengths");
        f5_run_checked(e, [&] {
            f5_ragged_loop(e, U, audio, text_ids, noise_in, seed, mem, pl);
            int64_t off = 0;
            for (int u = 0; u < U; ++u) {      // graph C per utterance, on its own frames of its slab
                const long len = e.decode(e.d_noise.as<float>() + (size_t)u * pl.Nmax * c.mel, 1, pl.Ns[u], pl.Rs[u], nullptr,
                                          e.v_outi.as<int16_t>());
                copy_out(out + off, e.v_outi.p, (size_t)len * 2, mem, e.stream);
                out_lens[u] = len;
                off += len;
            }
            MI_HIP(hipStreamSynchronize(e.stream));
        });
        e.finish_call();
    });
}

// mi_f5_synthesize_ragged up to the end of the loop, then utterance u's frames [R_u, N_u) of its slab as (100, N_u - R_u) channels first
int mi_f5_synthesize_mel_ragged(mi_f5* h, int U, const int16_t* audio, const int64_t* audio_lens, const int32_t* text_ids,
                                const int64_t* text_lens, const int64_t* max_durations, const float* noise_in, uint64_t seed, float* mel_out,
                                int64_t mel_cap, int64_t* n_frames, int mem) {
    return guard([&] {
        F5_CHECK(h, mem, "mi_f5_synthesize_mel_ragged");
        MI_REQUIRE(audio && text_ids && mel_out && n_frames && U >= 1, "mi_f5_synthesize_mel_ragged: bad arguments");
        F5& e = *h->impl;
        const F5Cfg& c = e.cfg;
        F5RaggedPlan pl = f5_ragged_plan(e, U, audio_lens, text_ids, text_lens, max_durations, mem, "mi_f5_synthesize_mel_ragged");
        int64_t total = 0;
        for (int u = 0; u < U; ++u) total += (int64_t)(pl.Ns[u] - pl.Rs[u]) * c.mel;
        MI_REQUIRE(total <= mel_cap, "mi_f5_synthesize_mel_ragged: mel_cap is smaller than the sum of the mels");
        f5_run_checked(e, [&] {
            f5_ragged_loop(e, U, audio, text_ids, noise_in, seed, mem, pl);
            float* dst = mel_out;
            if (mem == MI_HOST) { e.v_outf.ensure((size_t)total * 4); dst = e.v_outf.as<float>(); }
            int64_t off = 0;
            for (int u = 0; u < U; ++u) {
                const int F = pl.Ns[u] - pl.Rs[u];
                launch_nlc_to_ncl(e.d_noise.as<float>() + ((size_t)u * pl.Nmax + pl.Rs[u]) * c.mel, dst + off, 1, c.mel, F, MI_F32, e.stream);
                n_frames[u] = F;
                off += (int64_t)F * c.mel;
            }
            if (mem == MI_HOST) copy_out(mel_out, dst, (size_t)total * 4, mem, e.stream);
            MI_HIP(hipStreamSynchronize(e.stream));
        });
        e.finish_call();
    });
}

int mi_f5_dit_eval_ragged(mi_f5* h, int U, const int64_t* lens, const float* noise, const float* cmt, const float* cmtd, int64_t Nmax,
                          int k, float* pred, int mem) {
    return guard([&] {
        F5_CHECK(h, mem, "mi_f5_dit_eval_ragged");
        MI_REQUIRE(noise && cmt && cmtd && pred && U >= 1 && Nmax > 0 && Nmax <= h->impl->cfg.max_len, "mi_f5_dit_eval_ragged: bad arguments");
        F5& e = *h->impl;
        const int N = (int)Nmax;
        std::vector<int> Ls = f5_lengths(lens, U, 1, N, "mi_f5_dit_eval_ragged: lengths must be in [1, Nmax]");
        f5_run_checked(e, [&] {
            e.load_cond(noise, cmt, cmtd, U, N, mem);
            e.zero_pad_rows_cond(U, N, Ls.data());
            const int* dl = e.set_lengths(U, Ls.data());
            e.build_cat_cond(U, N);
            e.dit_eval(U, N, k, dl);
            MI_HIP(hipStreamSynchronize(e.stream));
        });
        copy_out(pred, e.pred_rows(U, N), (size_t)2 * U * N * e.cfg.mel * 4, mem, e.stream);
        MI_HIP(hipStreamSynchronize(e.stream));
        e.finish_call();
    });
}

int mi_f5_stft(mi_f5* h, const int16_t* audio, int64_t L, float* spec, int mem) {
    return guard([&] {
        F5_CHECK(h, mem, "mi_f5_stft");
        F5& e = *h->impl;
        MI_REQUIRE(audio && spec && L >= e.cfg.n_fft / 2 + 1 && L < (1L << 31), "mi_f5_stft: bad arguments");
        MI_HIP(hipSetDevice(e.device));
        const int nf = e.cfg.n_fft, nb = e.cfg.nb(), R = (int)(L / e.cfg.hop) + 1;
        e.p_audio.ensure((size_t)L * 2); e.p_pad.ensure((size_t)(L + nf) * 4 + 64); e.p_spec.ensure((size_t)R * 2 * nb * 4);
        const int16_t* da = audio;
        if (mem == MI_HOST) {
            MI_HIP(hipMemcpyAsync(e.p_audio.p, audio, (size_t)L * 2, hipMemcpyHostToDevice, e.stream));
            da = e.p_audio.as<int16_t>();
        }
        e.stft(da, 1, L);
        copy_out(spec, e.p_spec.p, (size_t)R * 2 * nb * 4, mem, e.stream);
        MI_HIP(hipStreamSynchronize(e.stream));
    });
}

// ---------------------------------------------------------------------------------------------------------------
// IndexTTS GPT
// ---------------------------------------------------------------------------------------------------------------
int64_t mi_gpt_param_count(const int32_t* cfg, int n_cfg) {
    int64_t n = -1;
    int rc = guard([&] { n = gpt_param_count(parse_gpt_cfg(cfg, n_cfg)); });
    return rc == MI_OK ? n : (int64_t)rc;
}

mi_gpt* mi_gpt_create(const int32_t* cfg, int n_cfg, const float* weights, int64_t n_weights, int dtype, int device) {
    mi_gpt* h = nullptr;
    int rc = guard([&] {
        MI_REQUIRE(weights != nullptr, "mi_gpt_create: null weights");
        GptCfg c = parse_gpt_cfg(cfg, n_cfg);
        Gpt* impl = new Gpt(c, weights, n_weights, dtype, device);
        h = new mi_gpt; h->impl = impl;
    });
    return rc == MI_OK ? h : nullptr;
}

mi_gpt* mi_gpt_create_mem(const int32_t* cfg, int n_cfg, const float* weights, int64_t n_weights, int dtype, int device,
                          int mem) {
    if (mem == MI_HOST) return mi_gpt_create(cfg, n_cfg, weights, n_weights, dtype, device);
    mi_gpt* h = nullptr;
    int rc = guard([&] {
        MI_REQUIRE(weights != nullptr && mem == MI_DEVICE, "mi_gpt_create_mem: null weights / bad mem kind");
        GptCfg c = parse_gpt_cfg(cfg, n_cfg);
        MI_REQUIRE(n_weights == gpt_param_count(c), "gpt: weight blob size does not match the config");
        std::vector<float> hw = read_back(weights, n_weights, device);
        Gpt* impl = new Gpt(c, hw.data(), n_weights, dtype, device);
        h = new mi_gpt; h->impl = impl;
    });
    return rc == MI_OK ? h : nullptr;
}

mi_gpt* mi_gpt_create_q8(const int32_t* cfg, int n_cfg, const float* weights, int64_t n_weights, int dtype, int device, int mem) {
    mi_gpt* h = nullptr;
    int rc = guard([&] {
        MI_REQUIRE(weights != nullptr && (mem == MI_HOST || mem == MI_DEVICE), "mi_gpt_create_q8: null weights / bad mem kind");
        GptCfg c = parse_gpt_cfg(cfg, n_cfg);
        MI_REQUIRE(n_weights == gpt_param_count(c), "gpt: weight blob size does not match the config");
        // quantised on the host from the fp32 blob, wherever it lives: the same bytes whichever mem
        std::vector<float> hw;
        if (mem == MI_DEVICE) hw = read_back(weights, n_weights, device);
        Gpt* impl = new Gpt(c, mem == MI_DEVICE ? hw.data() : weights, n_weights, dtype, device, GPT_W_Q8);
        h = new mi_gpt; h->impl = impl;
    });
    return rc == MI_OK ? h : nullptr;
}

int64_t mi_gpt_weight_bytes(mi_gpt* h) {
    int64_t n = -1;
    int rc = guard([&] {
        MI_REQUIRE(h && h->impl, "mi_gpt_weight_bytes: null handle");
        n = h->impl->weight_bytes();
    });
    return rc == MI_OK ? n : (int64_t)rc;
}

int mi_gpt_quantize_u8(const float* w, int n, int k, uint8_t* q, float* scale, uint8_t* zp) {
    return guard([&] {
        MI_REQUIRE(w && q && scale && zp, "mi_gpt_quantize_u8: null argument");
        MI_REQUIRE(n >= 1 && k >= 1 && (int64_t)n * k <= ((int64_t)1 << 40), "mi_gpt_quantize_u8: n and k must be positive");
        gpt_quantize_u8(w, n, k, q, scale, zp);
    });
}

void mi_gpt_destroy(mi_gpt* h) {
    if (!h) return;
    delete h->impl;                          // synchronises the stream: nothing of an open session is in flight afterwards
    delete h;                                // (an open session goes with it; it holds host memory only)
}

// Every entry on a GPT handle starts here, `who` being its name: the handle's lock, held while the result lives, the mem kind,
// the device.  no_session: the entry would touch the slots an open queue session decodes in.
static std::unique_lock<std::mutex> gpt_enter(mi_gpt* h, int mem, const std::string& who, bool no_session = false) {
    MI_REQUIRE(h && h->impl, who + ": null handle");
    std::unique_lock<std::mutex> lk(h->mu);
    MI_REQUIRE(mem == MI_HOST || mem == MI_DEVICE, who + ": bad mem kind");
    MI_HIP(hipSetDevice(h->impl->device));
    if (no_session && h->session) throw mi::Error(MI_ESTATE, who + ": a sentence-queue session is open on this handle (mi_gpt_queue_end)");
    return lk;
}

// input staged to the device when it lives on the host
static const void* stage_in(DevBuf& buf, const void* src, size_t bytes, int mem, hipStream_t s) {
    if (mem == MI_DEVICE) return src;
    buf.ensure(bytes);
    MI_HIP(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, s));
    return buf.p;
}

int mi_gpt_text_embed(mi_gpt* h, const int32_t* text_ids, int n, float* out, int mem) {
    return guard([&] {
        const auto lk_ = gpt_enter(h, mem, "mi_gpt_text_embed");
        Gpt& e = *h->impl;
        MI_REQUIRE(out && n >= 0 && (n == 0 || text_ids), "mi_gpt_text_embed: null argument");
        MI_REQUIRE(n + 2 <= e.cfg.max_text_pos, "mi_gpt_text_embed: text is longer than the text position table");
        if (mem == MI_HOST)
            for (int i = 0; i < n; ++i)
                MI_REQUIRE(text_ids[i] >= 0 && text_ids[i] < e.cfg.text_tokens, "mi_gpt_text_embed: text id out of range");
        const size_t ob = (size_t)(n + 2) * e.cfg.hidden * 4;
        const int32_t* ids = n ? (const int32_t*)stage_in(e.io_a, text_ids, (size_t)n * 4, mem, e.stream) : nullptr;
        float* o = out;
        if (mem == MI_HOST) { e.io_b.ensure(ob); o = e.io_b.as<float>(); }
        e.text_embed(ids, n, o);
        if (mem == MI_HOST) copy_out(out, o, ob, mem, e.stream);
        MI_HIP(hipStreamSynchronize(e.stream));
    });
}

int mi_gpt_mel_embed(mi_gpt* h, int32_t gpt_id, int64_t gen_len, float* out, int mem) {
    return guard([&] {
        const auto lk_ = gpt_enter(h, mem, "mi_gpt_mel_embed");
        Gpt& e = *h->impl;
        MI_REQUIRE(out != nullptr, "mi_gpt_mel_embed: null output");
        const size_t ob = (size_t)e.cfg.hidden * 4;
        float* o = out;
        if (mem == MI_HOST) { e.io_b.ensure(ob); o = e.io_b.as<float>(); }
        e.mel_embed(gpt_id, gen_len, o);
        if (mem == MI_HOST) copy_out(out, o, ob, mem, e.stream);
        MI_HIP(hipStreamSynchronize(e.stream));
    });
}

int mi_gpt_reset(mi_gpt* h) {
    return guard([&] {
        const auto lk_ = gpt_enter(h, MI_HOST, "mi_gpt_reset", true);
        h->impl->reset();
    });
}

int64_t mi_gpt_history_len(mi_gpt* h) {
    if (!h || !h->impl) return MI_EINVAL;
    return h->impl->history;
}

int mi_gpt_step(mi_gpt* h, const float* hidden_state, int ids_len, const float* repeat_penality, int attention_mask,
                float* last_hidden_state, int32_t* max_logit_id, float* logits, int mem) {
    return guard([&] {
        const auto lk_ = gpt_enter(h, mem, "mi_gpt_step", true);
        Gpt& e = *h->impl;
        const GptCfg& c = e.cfg;
        MI_REQUIRE(hidden_state && ids_len >= 1, "mi_gpt_step: hidden_state must hold at least one row");
        MI_REQUIRE(e.history + ids_len <= c.max_seq, "mi_gpt_step: history_len + ids_len exceeds the KV cache (max_seq)");
        hipStream_t s = e.stream;
        const hipMemcpyKind in = mem == MI_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
        MI_HIP(hipMemcpyAsync(e.X.p, hidden_state, (size_t)ids_len * c.hidden * 4, in, s));
        gpt_fill_penalty(e, 1, repeat_penality, in);
        std::vector<int32_t> w(GS_WORDS, 0);
        w[GS_HIST] = e.history;
        e.set_state(w);
        e.forward_rows(ids_len, attention_mask ? 1 : 0);
        copy_out(last_hidden_state, e.last.p, (size_t)c.hidden * 4, mem, s);
        copy_out(logits, e.logits.p, (size_t)c.mel_codes * 4, mem, s);      // un-penalised; see below
        copy_out(max_logit_id, e.state.as<int32_t>() + GS_TOKEN, 4, mem, s);
        w = e.get_state();                                                  // synchronises; history := hist + ids_len
    });
}

int mi_gpt_kv_read(mi_gpt* h, int layer, float* keys, float* values, int mem) {
    return guard([&] {
        const auto lk_ = gpt_enter(h, mem, "mi_gpt_kv_read");
        Gpt& e = *h->impl;
        const size_t n = (size_t)e.cfg.hidden * e.history * 4;
        if (n == 0) return;
        float *k = keys, *v = values;
        if (mem == MI_HOST) {
            e.io_a.ensure(n); e.io_b.ensure(n);
            k = keys ? e.io_a.as<float>() : nullptr; v = values ? e.io_b.as<float>() : nullptr;
        }
        e.kv_read(layer, k, v);
        if (mem == MI_HOST) { copy_out(keys, k, n, mem, e.stream); copy_out(values, v, n, mem, e.stream); }
        MI_HIP(hipStreamSynchronize(e.stream));
    });
}

int mi_gpt_kv_write(mi_gpt* h, int layer, const float* keys, const float* values, int hist, int mem) {
    return guard([&] {
        const auto lk_ = gpt_enter(h, mem, "mi_gpt_kv_write", true);
        Gpt& e = *h->impl;
        MI_REQUIRE(hist >= 0 && hist < e.cfg.max_seq, "mi_gpt_kv_write: history does not fit the KV cache (max_seq)");
        MI_REQUIRE(hist == 0 || (keys && values), "mi_gpt_kv_write: null keys/values");
        const size_t n = (size_t)e.cfg.hidden * hist * 4;
        const float* k = hist ? (const float*)stage_in(e.io_a, keys, n, mem, e.stream) : nullptr;
        const float* v = hist ? (const float*)stage_in(e.io_b, values, n, mem, e.stream) : nullptr;
        e.kv_write(layer, k, v, hist);
    });
}

static void gpt_generate_impl(mi_gpt* h, const float* prompt, int P, int max_new, const int32_t* stop_ids, int n_stop,
                              float repeat_value, int penalty_range, float* repeat_penality, int32_t* tokens, float* hidden,
                              int32_t* n_out, int mem, const GptSampleRec* rec, const std::string& who) {
    const auto lk_ = gpt_enter(h, mem, who, true);
    Gpt& e = *h->impl;
    const GptCfg& c = e.cfg;
    GptModeScope mode(e, rec, 1);
    MI_REQUIRE(prompt && P >= 1 && n_out, who + ": null argument");
    const std::vector<int32_t> stops = gpt_fetch_stops(stop_ids, n_stop, mem, who);
    *n_out = 0;
    if (max_new <= 0) return;                                        // `while num_decode < generate_limit` never runs
    gpt_check_lengths(c, 1, &P, &max_new, max_new, who);             // one sentence; the caller's buffers hold max_new rows
    hipStream_t s = e.stream;
    const hipMemcpyKind in = mem == MI_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    MI_HIP(hipMemcpyAsync(e.X.p, prompt, (size_t)P * c.hidden * 4, in, s));
    gpt_fill_penalty(e, 1, repeat_penality, in);
    e.set_rep_value(repeat_value);
    std::vector<int32_t> w = gpt_state_words(stops, penalty_range, 0, false);      // no limit word: the loop below counts
    e.set_state(w);
    e.forward_rows(P, 1);                                            // prompt pass: first token
    int left = max_new - 1;
    // the stop test needs the host: look at the state every `chunk` tokens (steps after a stop are no-ops)
    const int chunk = 16;
    for (;;) {
        w = e.get_state();
        if (w[GS_DONE] || left <= 0) break;
        const int n = left < chunk ? left : chunk;
        e.decode_steps(n);
        left -= n;
    }
    const int n = w[GS_NDEC];
    *n_out = n;
    copy_out(tokens, e.toks.p, (size_t)n * 4, mem, s);
    copy_out(hidden, e.hid.p, (size_t)n * c.hidden * 4, mem, s);
    copy_out(repeat_penality, e.pen.p, (size_t)c.mel_codes * 4, mem, s);
    MI_HIP(hipStreamSynchronize(s));
}

int mi_gpt_generate(mi_gpt* h, const float* prompt, int P, int max_new, const int32_t* stop_ids, int n_stop,
                    float repeat_value, int penalty_range, float* repeat_penality, int32_t* tokens, float* hidden,
                    int32_t* n_out, int mem) {
    return guard([&] {
        gpt_generate_impl(h, prompt, P, max_new, stop_ids, n_stop, repeat_value, penalty_range, repeat_penality, tokens, hidden,
                          n_out, mem, nullptr, "mi_gpt_generate");
    });
}

int mi_gpt_generate_sampled(mi_gpt* h, const float* prompt, int P, int max_new, const int32_t* stop_ids, int n_stop,
                            float repeat_value, int penalty_range, float* repeat_penality, int32_t* tokens, float* hidden,
                            int32_t* n_out, int mem, float temperature, int top_k, float top_p, uint64_t seed) {
    return guard([&] {
        const GptSampleRec rec = gpt_sample_rec(temperature, top_k, top_p, seed);
        gpt_generate_impl(h, prompt, P, max_new, stop_ids, n_stop, repeat_value, penalty_range, repeat_penality, tokens, hidden,
                          n_out, mem, &rec, "mi_gpt_generate_sampled");
    });
}

static void gpt_generate_batch_impl(mi_gpt* h, int nb, const float* prompts, const int32_t* prompt_rows, const int32_t* max_new,
                                    const int32_t* stop_ids, int n_stop, float repeat_value, int penalty_range,
                                    float* repeat_penality, int32_t* tokens, float* hidden, int cap, int32_t* n_out, int mem,
                                    const GptSampleRec* recs, const std::string& who) {
    const auto lk_ = gpt_enter(h, mem, who, true);
    Gpt& e = *h->impl;
    const GptCfg& c = e.cfg;
    MI_REQUIRE(prompts && prompt_rows && max_new && n_out && cap >= 1, who + ": null argument");
    MI_REQUIRE(nb >= 1 && nb <= c.max_batch, who + ": batch exceeds the handle's max_batch");
    GptModeScope mode(e, recs, nb);
    hipStream_t s = e.stream;
    const hipMemcpyKind in = mem == MI_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    const std::vector<int32_t> stops = gpt_fetch_stops(stop_ids, n_stop, mem, who);
    gpt_check_lengths(c, nb, prompt_rows, max_new, cap, who);
    gpt_fill_penalty(e, nb, repeat_penality, in);
    e.set_rep_value(repeat_value);
    bool any = false;
    size_t row0 = 0;
    for (int b = 0; b < nb; ++b) {                               // prompt passes, one sentence at a time
        e.set_state(gpt_state_words(stops, penalty_range, max_new[b], max_new[b] == 0), b);
        if (max_new[b] > 0) {
            MI_HIP(hipMemcpyAsync(e.X.p, prompts + row0 * c.hidden, (size_t)prompt_rows[b] * c.hidden * 4, in, s));
            e.forward_rows(prompt_rows[b], 1, b);
            any = true;
        }
        row0 += prompt_rows[b];
    }
    std::vector<int32_t> all((size_t)nb * GS_WORDS);
    int guard_steps = 0;
    while (any && !gpt_read_states(e, all)) {
        e.decode_batch_steps(nb, 16);
        guard_steps += 16;
        MI_REQUIRE(guard_steps <= c.max_seq + 32, who + ": decode loop did not terminate");
    }
    if (!any) gpt_read_states(e, all);
    e.history = all[GS_HIST];
    for (int b = 0; b < nb; ++b) {
        const int n = all[(size_t)b * GS_WORDS + GS_NDEC];
        n_out[b] = n;
        copy_out(tokens ? tokens + (size_t)b * cap : nullptr, e.toks.as<int32_t>() + (size_t)b * c.max_seq, (size_t)n * 4, mem, s);
        copy_out(hidden ? hidden + (size_t)b * cap * c.hidden : nullptr, e.hid.as<float>() + (size_t)b * c.max_seq * c.hidden,
                 (size_t)n * c.hidden * 4, mem, s);
    }
    copy_out(repeat_penality, e.pen.p, (size_t)nb * c.mel_codes * 4, mem, s);
    MI_HIP(hipStreamSynchronize(s));
}

int mi_gpt_generate_batch(mi_gpt* h, int nb, const float* prompts, const int32_t* prompt_rows, const int32_t* max_new,
                          const int32_t* stop_ids, int n_stop, float repeat_value, int penalty_range,
                          float* repeat_penality, int32_t* tokens, float* hidden, int cap, int32_t* n_out, int mem) {
    return guard([&] {
        gpt_generate_batch_impl(h, nb, prompts, prompt_rows, max_new, stop_ids, n_stop, repeat_value, penalty_range,
                                repeat_penality, tokens, hidden, cap, n_out, mem, nullptr, "mi_gpt_generate_batch");
    });
}

int mi_gpt_generate_batch_sampled(mi_gpt* h, int nb, const float* prompts, const int32_t* prompt_rows, const int32_t* max_new,
                                  const int32_t* stop_ids, int n_stop, float repeat_value, int penalty_range,
                                  float* repeat_penality, int32_t* tokens, float* hidden, int cap, int32_t* n_out, int mem,
                                  const float* temperature, const int32_t* top_k, const float* top_p, const uint64_t* seeds) {
    return guard([&] {
        MI_REQUIRE(nb >= 1 && nb <= 4096 && temperature && top_k && top_p && seeds, "mi_gpt_generate_batch_sampled: null argument");
        std::vector<GptSampleRec> recs(nb);
        for (int b = 0; b < nb; ++b) recs[b] = gpt_sample_rec(temperature[b], top_k[b], top_p[b], seeds[b]);
        gpt_generate_batch_impl(h, nb, prompts, prompt_rows, max_new, stop_ids, n_stop, repeat_value, penalty_range,
                                repeat_penality, tokens, hidden, cap, n_out, mem, recs.data(),
                                "mi_gpt_generate_batch_sampled");
    });
}

// Sentence queue (gpt_queue.h; include/mi355tts.h, "sentence queue"): the four entries that open one list their arguments as
// GptQueueArgs.  The blocking entries: a session driven to its end inside one call
static int gpt_queue_run(mi_gpt* h, const GptQueueArgs& a, int32_t* n_out, int32_t* stats) {
    return guard([&] {
        const auto lk_ = gpt_enter(h, a.mem, a.who, true);
        MI_REQUIRE(n_out != nullptr, std::string(a.who) + ": null argument");
        Gpt& e = *h->impl;
        GptQueue q(e, a);
        GptModeScope mode(e, q.sampled());
        GptBeamScope group(e, q.beams(), q.pool());
        while (q.round()) {}
        q.settle();
        q.report(n_out, nullptr, nullptr, stats);
    });
}

static int gpt_queue_open(mi_gpt* h, GptQueueArgs a) {
    return guard([&] {
        const auto lk_ = gpt_enter(h, a.mem, a.who, true);
        a.per_round = true;
        h->session.reset(new GptQueue(*h->impl, a));
    });
}

int mi_gpt_generate_queue(mi_gpt* h, int n, const float* prompts, const int32_t* prompt_rows, const int32_t* max_new,
                          const int32_t* stop_ids, int n_stop, float repeat_value, int penalty_range, int32_t* tokens,
                          float* hidden, int cap, int32_t* n_out, int mem, const float* temperature, const int32_t* top_k,
                          const float* top_p, const uint64_t* seeds, int32_t* stats) {
    return gpt_queue_run(h, {"mi_gpt_generate_queue", n, prompts, prompt_rows, max_new, stop_ids, n_stop, repeat_value, penalty_range,
                             tokens, hidden, cap, mem, temperature, top_k, top_p, seeds}, n_out, stats);
}

int mi_gpt_generate_queue_beam(mi_gpt* h, int n, const float* prompts, const int32_t* prompt_rows, const int32_t* max_new,
                               const int32_t* stop_ids, int n_stop, float repeat_value, int penalty_range, int num_beams,
                               int32_t* tokens, float* hidden, int cap, int32_t* n_out, float* scores, int mem, int32_t* stats) {
    return gpt_queue_run(h, {"mi_gpt_generate_queue_beam", n, prompts, prompt_rows, max_new, stop_ids, n_stop, repeat_value, penalty_range,
                             tokens, hidden, cap, mem, nullptr, nullptr, nullptr, nullptr, true, num_beams, scores}, n_out, stats);
}

int mi_gpt_queue_begin(mi_gpt* h, int n, const float* prompts, const int32_t* prompt_rows, const int32_t* max_new,
                       const int32_t* stop_ids, int n_stop, float repeat_value, int penalty_range, int32_t* tokens, float* hidden,
                       int cap, int mem, const float* temperature, const int32_t* top_k, const float* top_p, const uint64_t* seeds) {
    return gpt_queue_open(h, {"mi_gpt_queue_begin", n, prompts, prompt_rows, max_new, stop_ids, n_stop, repeat_value, penalty_range,
                              tokens, hidden, cap, mem, temperature, top_k, top_p, seeds});
}

int mi_gpt_queue_begin_beam(mi_gpt* h, int n, const float* prompts, const int32_t* prompt_rows, const int32_t* max_new,
                            const int32_t* stop_ids, int n_stop, float repeat_value, int penalty_range, int num_beams,
                            int32_t* tokens, float* hidden, int cap, float* scores, int mem) {
    return gpt_queue_open(h, {"mi_gpt_queue_begin_beam", n, prompts, prompt_rows, max_new, stop_ids, n_stop, repeat_value, penalty_range,
                              tokens, hidden, cap, mem, nullptr, nullptr, nullptr, nullptr, true, num_beams, scores});
}

// pool mode through the queue: the beam entries' arguments, the search's parameters and the four sampling arrays (all or none)
int mi_gpt_generate_queue_beam_pool(mi_gpt* h, int n, const float* prompts, const int32_t* prompt_rows, const int32_t* max_new,
                                    const int32_t* stop_ids, int n_stop, float repeat_value, int penalty_range, int num_beams,
                                    float length_penalty, int early_stopping, const float* temperature, const int32_t* top_k,
                                    const float* top_p, const uint64_t* seeds, int32_t* tokens, float* hidden, int cap,
                                    int32_t* n_out, float* scores, int mem, int32_t* stats) {
    return gpt_queue_run(h, {"mi_gpt_generate_queue_beam_pool", n, prompts, prompt_rows, max_new, stop_ids, n_stop, repeat_value,
                             penalty_range, tokens, hidden, cap, mem, temperature, top_k, top_p, seeds, true, num_beams, scores, true,
                             length_penalty, early_stopping}, n_out, stats);
}

int mi_gpt_queue_begin_beam_pool(mi_gpt* h, int n, const float* prompts, const int32_t* prompt_rows, const int32_t* max_new,
                                 const int32_t* stop_ids, int n_stop, float repeat_value, int penalty_range, int num_beams,
                                 float length_penalty, int early_stopping, const float* temperature, const int32_t* top_k,
                                 const float* top_p, const uint64_t* seeds, int32_t* tokens, float* hidden, int cap, float* scores,
                                 int mem) {
    return gpt_queue_open(h, {"mi_gpt_queue_begin_beam_pool", n, prompts, prompt_rows, max_new, stop_ids, n_stop, repeat_value,
                              penalty_range, tokens, hidden, cap, mem, temperature, top_k, top_p, seeds, true, num_beams, scores, true,
                              length_penalty, early_stopping});
}

int mi_gpt_queue_advance(mi_gpt* h, int32_t* count, int32_t* done, int32_t* finished, int32_t* stats) {
    return guard([&] {
        const std::string who = "mi_gpt_queue_advance";
        const auto lk_ = gpt_enter(h, MI_HOST, who);
        if (!h->session) throw mi::Error(MI_ESTATE, who + ": no session is open on this handle");
        MI_REQUIRE(count && done && finished, who + ": null argument");
        Gpt& e = *h->impl;
        GptQueue& q = *h->session;
        if (!q.ended()) {
            GptModeScope mode(e, q.sampled());
            GptBeamScope group(e, q.beams(), q.pool());
            if (q.round()) q.publish_live();
            q.settle();
        }
        q.report(count, done, finished, stats);
    });
}

int mi_gpt_queue_end(mi_gpt* h) {
    return guard([&] {
        const auto lk_ = gpt_enter(h, MI_HOST, "mi_gpt_queue_end");
        if (!h->session) throw mi::Error(MI_ESTATE, "mi_gpt_queue_end: no session is open on this handle");
        (void)hipStreamSynchronize(h->impl->stream);                 // nothing of the session is in flight when its arrays go
        h->session.reset();
    });
}

// tests and tools: the queue's policy object driven on the host alone; no handle, no GPU
int mi_gpt_queue_schedule(int n, const int32_t* prompt_rows, const int32_t* max_new, const int32_t* lengths, int slots, int max_seq,
                          int beams, int32_t* steps, int32_t* n_passes, int32_t* pass_of, int32_t* unit_of) {
    return guard([&] { gpt_queue_schedule(n, prompt_rows, max_new, lengths, slots, max_seq, beams, steps, n_passes, pass_of, unit_of); });
}

// beam search (gpt_beam.hip, gpt_beam_pool.hip): gpt_generate_batch_impl's loop over nb groups of B slots, behind both beam
// entries.  pool == null: hypothesis 0 is the result and its penalty vector is written back; else the pool-mode selection runs
// and pool entry 0 is the result.
struct GptPoolCall { float length_penalty; int early_stopping; const float* temperature; const int32_t* top_k; const float* top_p; const uint64_t* seeds; };

static void gpt_beam_run(mi_gpt* h, const std::string& who, int nb, const float* prompts, const int32_t* prompt_rows,
                         const int32_t* max_new, const int32_t* stop_ids, int n_stop, float repeat_value, int penalty_range,
                         const float* pen_in, float* pen_out, int num_beams, const GptPoolCall* pool, int32_t* tokens, float* hidden,
                         int cap, int32_t* n_out, float* scores, int mem) {
    const auto lk_ = gpt_enter(h, mem, who, true);
    Gpt& e = *h->impl;
    const GptCfg& c = e.cfg;
    const int B = num_beams;
    MI_REQUIRE(prompts && prompt_rows && max_new && n_out && cap >= 1, who + ": null argument");
    MI_REQUIRE(B >= 1 && B <= GPT_BEAM_MAX, who + ": num_beams must be in [1, 8]");
    MI_REQUIRE(B <= c.mel_codes, who + ": num_beams exceeds the mel codes");
    MI_REQUIRE(nb >= 1 && (long)nb * B <= c.max_batch, who + ": nb * num_beams exceeds the handle's max_batch");
    bool sampling = false;
    if (pool) {
        MI_REQUIRE(std::isfinite(pool->length_penalty), who + ": length_penalty must be finite");
        MI_REQUIRE(pool->early_stopping == 0 || pool->early_stopping == 1, who + ": early_stopping must be 0 or 1");
        sampling = pool->temperature || pool->top_k || pool->top_p || pool->seeds;
        MI_REQUIRE(!sampling || (pool->temperature && pool->top_k && pool->top_p && pool->seeds), who + ": the four sampling arrays go together");
    }
    hipStream_t s = e.stream;
    const hipMemcpyKind in = mem == MI_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    const std::vector<int32_t> stops = gpt_fetch_stops(stop_ids, n_stop, mem, who);
    std::vector<GptSampleRec> recs;
    if (pool) {
        const int K = ((int)stops.size() + 1) * B;
        MI_REQUIRE(K <= GPT_POOL_MAX_CAND && K <= c.mel_codes, who + ": (n_stop + 1) * num_beams must be <= 64 and <= mel_codes");
        if (sampling) {
            MI_REQUIRE(c.mel_codes <= GPT_SAMPLE_MAX_CODES, who + ": sampling supports at most 16384 mel codes");
            for (int g = 0; g < nb; ++g) {
                recs.push_back(gpt_sample_rec(pool->temperature[g], pool->top_k[g], pool->top_p[g], pool->seeds[g]));
                MI_REQUIRE(pool->top_k[g] == 0 || pool->top_k[g] >= K, who + ": top_k must be 0 or at least (n_stop + 1) * num_beams");
            }
        }
    }
    gpt_check_lengths(c, nb, prompt_rows, max_new, cap, who);
    GptBeamScope group(e, B);
    e.sampled = 0;
    if (pool) e.pool_ensure(); else e.beam_ensure();
    const int nr = nb * B;
    // pen0 of sentence g -> side 0 of the group's first slot (selection 0 reads it there)
    gpt_fill_penalty(e, nb, pen_in, in, B);
    e.set_rep_value(repeat_value);
    if (pool) e.pool_begin(nb, B, GptPoolCfg{pool->length_penalty, pool->early_stopping, sampling ? 1 : 0, 0}, sampling ? recs.data() : nullptr);
    std::vector<int32_t> all((size_t)nr * GS_WORDS, 0);
    for (int g = 0; g < nb; ++g) {
        const std::vector<int32_t> w = gpt_state_words(stops, penalty_range, max_new[g], max_new[g] == 0);
        for (int i = 0; i < B; ++i) std::copy(w.begin(), w.end(), all.begin() + ((size_t)g * B + i) * GS_WORDS);
    }
    MI_HIP(hipMemcpyAsync(e.state.p, all.data(), all.size() * 4, hipMemcpyHostToDevice, s));
    MI_HIP(hipStreamSynchronize(s));
    e.history = 0;
    bool any = false;
    size_t row0 = 0;
    for (int g = 0; g < nb; ++g) {                               // prompt passes, one per sentence, into the group's first slot
        if (max_new[g] > 0) {
            MI_HIP(hipMemcpyAsync(e.X.p, prompts + row0 * c.hidden, (size_t)prompt_rows[g] * c.hidden * 4, in, s));
            e.forward_rows(prompt_rows[g], 1, g * B);
            if (pool) e.pool_select_first(g, B, prompt_rows[g]); else e.beam_select_first(g, B, prompt_rows[g]);
            any = true;
        }
        row0 += prompt_rows[g];
    }
    int guard_steps = 0;
    while (any && !gpt_read_states(e, all, B)) {
        if (pool) e.decode_pool_steps(nb, B, 16); else e.decode_beam_steps(nb, B, 16);
        guard_steps += 16;
        MI_REQUIRE(guard_steps <= c.max_seq + 32, who + ": decode loop did not terminate");
    }
    if (!any) gpt_read_states(e, all, B);
    e.history = all[GS_HIST];
    // the result of every group (hypothesis 0 along its ancestors, or pool entry 0 along its frozen list), gathered into
    // staging, then out like the batched entry's rows
    std::vector<int32_t> meta;
    if (pool) {
        meta.resize((size_t)nr * GPT_POOL_META);
        MI_HIP(hipMemcpyAsync(meta.data(), e.pool_meta.p, meta.size() * 4, hipMemcpyDeviceToHost, s));
        MI_HIP(hipStreamSynchronize(s));
    }
    e.io_a.ensure((size_t)nb * cap * 4);
    if (hidden) e.io_b.ensure((size_t)nb * cap * c.hidden * 4);
    if (pool) e.pool_gather(nb, B, e.io_a.as<int32_t>(), hidden ? e.io_b.as<float>() : nullptr, cap);
    else e.beam_gather(nb, B, e.io_a.as<int32_t>(), hidden ? e.io_b.as<float>() : nullptr, cap);
    for (int g = 0; g < nb; ++g) {
        const size_t s0 = (size_t)g * B;
        int n = all[s0 * GS_WORDS + GS_NDEC];
        if (pool) {
            const int32_t* mw = meta.data() + s0 * GPT_POOL_META;
            n = mw[PM_FIN] ? std::min(std::max(mw[PM_LEN], 0), cap) : 0;
        }
        n_out[g] = n;
        copy_out(tokens ? tokens + (size_t)g * cap : nullptr, e.io_a.as<int32_t>() + (size_t)g * cap, (size_t)n * 4, mem, s);
        if (hidden)
            copy_out(hidden + (size_t)g * cap * c.hidden, e.io_b.as<float>() + (size_t)g * cap * c.hidden,
                     (size_t)n * c.hidden * 4, mem, s);
        if (pool) {
            if (n == 0) MI_HIP(hipMemsetAsync(e.pool_score.as<float>() + s0, 0, 4, s));      // nothing returned: score 0, not the empty pool's -1e9
            copy_out(scores ? scores + g : nullptr, e.pool_score.as<float>() + s0, 4, mem, s);
        } else {
            const int nd = all[s0 * GS_WORDS + GS_NDEC];
            const float* pen_side = ((nd & 1) ? e.pen_b.as<float>() : e.pen.as<float>()) + s0 * c.mel_codes;
            copy_out(pen_out ? pen_out + (size_t)g * c.mel_codes : nullptr, pen_side, (size_t)c.mel_codes * 4, mem, s);
            copy_out(scores ? scores + g : nullptr, e.score.as<float>() + s0, 4, mem, s);
        }
    }
    MI_HIP(hipStreamSynchronize(s));
}

int mi_gpt_generate_beam(mi_gpt* h, int nb, const float* prompts, const int32_t* prompt_rows, const int32_t* max_new,
                         const int32_t* stop_ids, int n_stop, float repeat_value, int penalty_range, float* repeat_penality,
                         int num_beams, int32_t* tokens, float* hidden, int cap, int32_t* n_out, float* scores, int mem) {
    return guard([&] {
        gpt_beam_run(h, "mi_gpt_generate_beam", nb, prompts, prompt_rows, max_new, stop_ids, n_stop, repeat_value, penalty_range,
                     repeat_penality, repeat_penality, num_beams, nullptr, tokens, hidden, cap, n_out, scores, mem);
    });
}

int mi_gpt_beam_select(const float* logits, const float* pen, const float* prev_scores, int groups, int beams, int codes,
                       int first, int32_t* parents, int32_t* tokens, float* scores, int mem) {
    return guard([&] {
        MI_REQUIRE(mem == MI_HOST || mem == MI_DEVICE, "mi_gpt_beam_select: bad mem kind");
        MI_REQUIRE(logits && (first || prev_scores) && parents && tokens && scores, "mi_gpt_beam_select: null argument");
        MI_REQUIRE(groups >= 1 && groups <= (1 << 20), "mi_gpt_beam_select: groups");
        MI_REQUIRE(codes >= 1 && codes <= GPT_BEAM_MAX_CODES, "mi_gpt_beam_select: supports 1..16384 codes");
        MI_REQUIRE(beams >= 1 && beams <= GPT_BEAM_MAX && beams <= codes, "mi_gpt_beam_select: beams must be in [1, 8] and <= codes");
        hipStream_t s;
        MI_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        struct Fin { hipStream_t s; ~Fin() { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } } fin{s};
        DevBuf dl, dp, dv, dpar, dtok, dsc;
        const size_t rows = (size_t)groups * beams, n = rows * codes;
        const float* l = (const float*)stage_in(dl, logits, n * 4, mem, s);
        const float* p = pen ? (const float*)stage_in(dp, pen, n * 4, mem, s) : nullptr;
        const float* v = first ? nullptr : (const float*)stage_in(dv, prev_scores, rows * 4, mem, s);
        int32_t *par = parents, *tok = tokens;
        float* sc = scores;
        if (mem == MI_HOST) {
            dpar.ensure(rows * 4); dtok.ensure(rows * 4); dsc.ensure(rows * 4);
            par = dpar.as<int32_t>(); tok = dtok.as<int32_t>(); sc = dsc.as<float>();
        }
        launch_gpt_beam_select_rows(l, p, v, groups, beams, codes, first, par, tok, sc, s);
        if (mem == MI_HOST) {
            copy_out(parents, par, rows * 4, mem, s);
            copy_out(tokens, tok, rows * 4, mem, s);
            copy_out(scores, sc, rows * 4, mem, s);
        }
        MI_HIP(hipStreamSynchronize(s));
    });
}

// beam search with a finished pool (gpt_beam_pool.hip): the same loop with the pool-mode selection
int mi_gpt_generate_beam_pool(mi_gpt* h, int nb, const float* prompts, const int32_t* prompt_rows, const int32_t* max_new,
                              const int32_t* stop_ids, int n_stop, float repeat_value, int penalty_range,
                              const float* repeat_penality, int num_beams, float length_penalty, int early_stopping,
                              const float* temperature, const int32_t* top_k, const float* top_p, const uint64_t* seeds,
                              int32_t* tokens, float* hidden, int cap, int32_t* n_out, float* scores, int mem) {
    return guard([&] {
        const GptPoolCall pc{length_penalty, early_stopping, temperature, top_k, top_p, seeds};
        gpt_beam_run(h, "mi_gpt_generate_beam_pool", nb, prompts, prompt_rows, max_new, stop_ids, n_stop, repeat_value, penalty_range,
                     repeat_penality, nullptr, num_beams, &pc, tokens, hidden, cap, n_out, scores, mem);
    });
}

int mi_gpt_beam_pool_select(const float* logits, const float* pen, const float* prev_scores, int beams, int codes, int n,
                            int max_new, const int32_t* stop_ids, int n_stop, float* pool_scores, int32_t* pool_finished,
                            int32_t* open, float length_penalty, int early_stopping, const float* temperature,
                            const int32_t* top_k, const float* top_p, const uint64_t* seed, int32_t* cand, float* cand_acc,
                            int32_t* cand_stop, int32_t* parents, int32_t* tokens, float* scores, int32_t* pool_src,
                            int32_t* done, int mem) {
    return guard([&] {
        const std::string who = "mi_gpt_beam_pool_select";
        MI_REQUIRE(mem == MI_HOST || mem == MI_DEVICE, who + ": bad mem kind");
        MI_REQUIRE(logits && (n == 0 || prev_scores) && pool_scores && pool_finished && open && cand && cand_acc && cand_stop &&
                   parents && tokens && scores && pool_src && done, who + ": null argument");
        MI_REQUIRE(codes >= 1 && codes <= GPT_BEAM_MAX_CODES, who + ": supports 1..16384 codes");
        MI_REQUIRE(beams >= 1 && beams <= GPT_BEAM_MAX, who + ": beams must be in [1, 8]");
        MI_REQUIRE(n_stop >= 0 && n_stop <= GS_WORDS - GS_STOP0 && (n_stop == 0 || stop_ids), who + ": at most 6 stop ids");
        MI_REQUIRE(n >= 0 && max_new >= 1 && n < max_new, who + ": 0 <= n < max_new");
        MI_REQUIRE(std::isfinite(length_penalty), who + ": length_penalty must be finite");
        MI_REQUIRE(early_stopping == 0 || early_stopping == 1, who + ": early_stopping must be 0 or 1");
        const int B = beams, K = (n_stop + 1) * B;
        MI_REQUIRE(K <= GPT_POOL_MAX_CAND && K <= codes, who + ": (n_stop + 1) * beams must be <= 64 and <= codes");
        const bool sampling = temperature || top_k || top_p || seed;
        MI_REQUIRE(!sampling || (temperature && top_k && top_p && seed), who + ": the four sampling parameters go together");
        GptPoolSelect p{};
        p.B = B; p.codes = codes; p.n = n; p.max_new = max_new; p.n_stop = n_stop;
        for (int q = 0; q < n_stop; ++q) p.stops[q] = stop_ids[q];
        p.length_penalty = length_penalty; p.early_stopping = early_stopping; p.sampling = sampling ? 1 : 0;
        p.rec = GptSampleRec{1.f, 1.f, 0, 0u, 0u, {0u, 0u, 0u}};
        if (sampling) {
            p.rec = gpt_sample_rec(*temperature, *top_k, *top_p, *seed);
            MI_REQUIRE(*top_k == 0 || *top_k >= K, who + ": top_k must be 0 or at least (n_stop + 1) * beams");
        }
        hipStream_t s;
        MI_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        struct Fin { hipStream_t s; ~Fin() { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } } fin{s};
        DevBuf dl, dp, dkeys, dsmall;
        const size_t nl = (size_t)B * codes;
        const float* l = (const float*)stage_in(dl, logits, nl * 4, mem, s);
        const float* pn = pen ? (const float*)stage_in(dp, pen, nl * 4, mem, s) : nullptr;
        dkeys.ensure(nl * 4);
        // the small arrays are HOST arrays: one staging block, words [prev B | pool_score B | pool_fin B | open, done | cand K |
        // cand_acc K | cand_stop K | parents B | tokens B | scores B | pool_src B]
        const size_t words = 7 * (size_t)B + 2 + 3 * (size_t)K;
        std::vector<int32_t> hb(words, 0);
        float* hf = reinterpret_cast<float*>(hb.data());
        for (int b = 0; b < B; ++b) {
            hf[b] = n == 0 ? 0.f : prev_scores[b];
            hf[B + b] = pool_scores[b];
            hb[2 * B + b] = pool_finished[b] != 0;
        }
        hb[3 * B] = *open != 0;
        dsmall.ensure(words * 4);
        MI_HIP(hipMemcpyAsync(dsmall.p, hb.data(), words * 4, hipMemcpyHostToDevice, s));
        int32_t* d = dsmall.as<int32_t>();
        float* df = dsmall.as<float>();
        const size_t oc = 3 * (size_t)B + 2, ob = oc + 3 * (size_t)K;
        launch_gpt_pool_select(l, pn, dkeys.as<unsigned>(), p, df, df + B, d + 2 * B, d + 3 * B, d + oc, df + oc + K, d + oc + 2 * K,
                               d + ob, d + ob + B, df + ob + 2 * B, d + ob + 3 * B, s);
        MI_HIP(hipMemcpyAsync(hb.data(), dsmall.p, words * 4, hipMemcpyDeviceToHost, s));
        MI_HIP(hipStreamSynchronize(s));
        for (int b = 0; b < B; ++b) {
            pool_scores[b] = hf[B + b]; pool_finished[b] = hb[2 * B + b];
            parents[b] = hb[ob + b]; tokens[b] = hb[ob + B + b]; scores[b] = hf[ob + 2 * B + b]; pool_src[b] = hb[ob + 3 * B + b];
        }
        *open = hb[3 * B]; *done = hb[3 * B + 1];
        for (int q = 0; q < K; ++q) { cand[q] = hb[oc + q]; cand_acc[q] = hf[oc + K + q]; cand_stop[q] = hb[oc + 2 * K + q]; }
    });
}

int mi_gpt_bench_pick(mi_gpt* h, int nb, int iters, const float* temperature, const int32_t* top_k, const float* top_p,
                      double* us) {
    return guard([&] {
        const auto lk_ = gpt_enter(h, MI_HOST, "mi_gpt_bench_pick", true);
        Gpt& e = *h->impl;
        MI_REQUIRE(us && nb >= 1 && nb <= e.cfg.max_batch && iters >= 1, "mi_gpt_bench_pick: bad arguments");
        std::vector<GptSampleRec> recs;
        if (temperature) {
            MI_REQUIRE(top_k && top_p, "mi_gpt_bench_pick: null argument");
            for (int b = 0; b < nb; ++b) recs.push_back(gpt_sample_rec(temperature[b], top_k[b], top_p[b], 1 + b));
        }
        GptModeScope mode(e, temperature ? recs.data() : nullptr, nb);
        *us = e.bench_pick(nb, iters);
    });
}

int mi_gpt_sample_logits(const float* logits, const float* pen, int rows, int codes, const float* temperature,
                         const int32_t* top_k, const float* top_p, const uint64_t* seeds, const int64_t* positions,
                         int32_t* tokens, float* u_out, float* prob_out, int mem) {
    return guard([&] {
        MI_REQUIRE(mem == MI_HOST || mem == MI_DEVICE, "mi_gpt_sample_logits: bad mem kind");
        MI_REQUIRE(logits && temperature && top_k && top_p && seeds && positions && tokens && u_out, "mi_gpt_sample_logits: null argument");
        MI_REQUIRE(rows >= 1 && rows <= (1 << 20), "mi_gpt_sample_logits: rows");
        MI_REQUIRE(codes >= 1 && codes <= GPT_SAMPLE_MAX_CODES, "mi_gpt_sample_logits: sampling supports 1..16384 codes");
        std::vector<GptSampleRec> recs(rows);
        for (int r = 0; r < rows; ++r) {
            recs[r] = gpt_sample_rec(temperature[r], top_k[r], top_p[r], seeds[r]);
            MI_REQUIRE(positions[r] >= 0, "mi_gpt_sample_logits: positions must be >= 0");
        }
        hipStream_t s;
        MI_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        struct Fin { hipStream_t s; ~Fin() { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } } fin{s};
        DevBuf drec, dpos, dl, dp, dt, du, dpr;
        const size_t n = (size_t)rows * codes;
        drec.ensure(recs.size() * sizeof(GptSampleRec)); dpos.ensure((size_t)rows * 8);
        MI_HIP(hipMemcpyAsync(drec.p, recs.data(), recs.size() * sizeof(GptSampleRec), hipMemcpyHostToDevice, s));
        MI_HIP(hipMemcpyAsync(dpos.p, positions, (size_t)rows * 8, hipMemcpyHostToDevice, s));
        const float* l = (const float*)stage_in(dl, logits, n * 4, mem, s);
        const float* p = pen ? (const float*)stage_in(dp, pen, n * 4, mem, s) : nullptr;
        int32_t* t = tokens; float* u = u_out; float* pr = prob_out;
        if (mem == MI_HOST) {
            dt.ensure((size_t)rows * 4); du.ensure((size_t)rows * 4);
            t = dt.as<int32_t>(); u = du.as<float>();
            if (prob_out) { dpr.ensure(n * 4); pr = dpr.as<float>(); }
        }
        launch_gpt_sample_rows(l, p, rows, codes, drec.as<GptSampleRec>(), dpos.as<int64_t>(), t, u, pr, s);
        if (mem == MI_HOST) {
            copy_out(tokens, t, (size_t)rows * 4, mem, s);
            copy_out(u_out, u, (size_t)rows * 4, mem, s);
            if (prob_out) copy_out(prob_out, pr, n * 4, mem, s);
        }
        MI_HIP(hipStreamSynchronize(s));
    });
}

}  // extern "C"

// The unit entries of the four attention launches share this: fp32 inputs staged and rounded to `dtype` on the device, the
// GS_* state words built from the host tables, the engine's launcher (gpt.h), the output back as fp32.  The output is preset
// to NaN bytes, so a row the launch does not write shows.
namespace {
struct AttnUnit {
    hipStream_t s = nullptr;
    int dtype, heads, hidden, max_seq;
    DevBuf in_q, in_k, in_v, q, k, v, o, o32, st;
    AttnUnit(const std::string& who, int dt, int heads_, int max_seq_, int mem) : dtype(dt), heads(heads_), hidden(64 * heads_), max_seq(max_seq_) {
        MI_REQUIRE(mem == MI_HOST || mem == MI_DEVICE, who + ": bad mem kind");
        MI_REQUIRE(dt == MI_F32 || dt == MI_F16 || dt == MI_BF16, who + ": dtype must be MI_F32, MI_F16 or MI_BF16");
        MI_REQUIRE(heads_ >= 1 && heads_ <= 64, who + ": heads must be in [1, 64] (hidden = 64 * heads)");
        // the dynamic LDS of the prompt kernels stays below what a launch may ask for without raising the function attribute
        MI_REQUIRE(max_seq_ >= 1 && max_seq_ <= 8192, who + ": max_seq must be in [1, 8192]");
        MI_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    }
    ~AttnUnit() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
    size_t slot_elems() const { return (size_t)hidden * max_seq; }
    void inputs(const float* qkv, int rows, const float* kc, const float* vc, int nslots, int mem) {
        const size_t es = dtype_size(dtype), nq = (size_t)rows * 3 * hidden, nc = (size_t)nslots * slot_elems();
        q.ensure(nq * es); k.ensure(nc * es); v.ensure(nc * es); o.ensure((size_t)rows * hidden * es);
        launch_copy2d((const float*)stage_in(in_q, qkv, nq * 4, mem, s), 3 * hidden, q.p, 3 * hidden, rows, 3 * hidden, dtype, s);
        launch_copy2d((const float*)stage_in(in_k, kc, nc * 4, mem, s), 64, k.p, 64, (long)(nc / 64), 64, dtype, s);
        launch_copy2d((const float*)stage_in(in_v, vc, nc * 4, mem, s), 64, v.p, 64, (long)(nc / 64), 64, dtype, s);
        MI_HIP(hipMemsetAsync(o.p, 0xFF, (size_t)rows * hidden * es, s));
    }
    // words[slot] = (GS_HIST, GS_NDEC)
    void state(const std::vector<std::pair<int, int>>& words) {
        std::vector<int32_t> w(words.size() * GS_WORDS, 0);
        for (size_t b = 0; b < words.size(); ++b) { w[b * GS_WORDS + GS_HIST] = words[b].first; w[b * GS_WORDS + GS_NDEC] = words[b].second; }
        st.ensure(w.size() * 4);
        MI_HIP(hipMemcpyAsync(st.p, w.data(), w.size() * 4, hipMemcpyHostToDevice, s));
        MI_HIP(hipStreamSynchronize(s));       // `w` is a local
    }
    void result(float* out, int rows, int mem) {
        const size_t n = (size_t)rows * hidden;
        float* dst = out;
        if (mem == MI_HOST) { o32.ensure(n * 4); dst = o32.as<float>(); }
        launch_cast_to_f32(o.p, dtype, dst, (long)n, s);
        if (mem == MI_HOST) copy_out(out, dst, n * 4, mem, s);
        MI_HIP(hipStreamSynchronize(s));
    }
};

// The unit entries of the decode-step linear launches share this: a stream of their own, fp32 arrays staged (and rounded to
// `dtype` where the engine holds them so), NaN-preset outputs, results widened back.
struct LinUnit {
    hipStream_t s = nullptr;
    int dtype, mem;
    std::vector<std::unique_ptr<DevBuf>> bufs;
    LinUnit(const std::string& who, int dt, int mem_) : dtype(dt), mem(mem_) {
        MI_REQUIRE(mem == MI_HOST || mem == MI_DEVICE, who + ": bad mem kind");
        MI_REQUIRE(dt == MI_F32 || dt == MI_F16 || dt == MI_BF16, who + ": dtype must be MI_F32, MI_F16 or MI_BF16");
        MI_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    }
    ~LinUnit() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
    DevBuf& buf(size_t bytes) { bufs.emplace_back(new DevBuf); bufs.back()->ensure(bytes); return *bufs.back(); }
    // n fp32 values of the caller, on the device (null stays null)
    const float* f32(const float* p, size_t n) {
        if (!p || mem == MI_DEVICE) return p;
        bufs.emplace_back(new DevBuf);
        return (const float*)stage_in(*bufs.back(), p, n * 4, mem, s);
    }
    // n bytes of the caller, on the device
    const void* bytes(const void* p, size_t n) {
        if (mem == MI_DEVICE) return p;
        bufs.emplace_back(new DevBuf);
        return stage_in(*bufs.back(), p, n, mem, s);
    }
    // (rows, cols) fp32 of the caller -> rows [0, rows) of a device array of `dt` with alloc_rows >= rows rows
    void* typed(const float* p, long rows, int cols, int dt, long alloc_rows = 0) {
        DevBuf& d = buf((size_t)std::max(rows, alloc_rows) * cols * dtype_size(dt));
        launch_copy2d(f32(p, (size_t)rows * cols), cols, d.p, cols, rows, cols, dt, s);
        return d.p;
    }
    // n elements of `dt`, every byte 0xFF (a NaN in all three types)
    void* nan_out(size_t n, int dt) {
        DevBuf& d = buf(n * dtype_size(dt));
        MI_HIP(hipMemsetAsync(d.p, 0xFF, n * dtype_size(dt), s));
        return d.p;
    }
    // n elements of `dt` on the device -> the caller's fp32 array (null: not wanted)
    void give(float* dst, const void* src, size_t n, int dt) {
        if (!dst) return;
        float* d = mem == MI_HOST ? (float*)buf(n * 4).p : dst;
        launch_cast_to_f32(src, dt, d, (long)n, s);
        if (mem == MI_HOST) copy_out(dst, d, n * 4, mem, s);
    }
    const int* state(const int32_t* hist, int nslots, int rows) {
        std::vector<int32_t> w((size_t)rows * GS_WORDS, 0);
        for (int b = 0; b < nslots; ++b) w[(size_t)b * GS_WORDS + GS_HIST] = hist ? hist[b] : 0;
        DevBuf& d = buf(w.size() * 4);
        MI_HIP(hipMemcpyAsync(d.p, w.data(), w.size() * 4, hipMemcpyHostToDevice, s));
        MI_HIP(hipStreamSynchronize(s));       // `w` is a local
        return d.as<int>();
    }
};
}  // namespace

extern "C" {

int mi_gpt_attn_decode(const float* qkv, const float* kc, const float* vc, int dtype, int heads, int max_seq, int nslots,
                       const int32_t* hist, float* out, int mem) {
    return guard([&] {
        const std::string who = "mi_gpt_attn_decode";
        AttnUnit u(who, dtype, heads, max_seq, mem);
        MI_REQUIRE(qkv && kc && vc && hist && out, who + ": null argument");
        MI_REQUIRE(nslots >= 1 && nslots <= GPT_MAX_BATCH, who + ": nslots must be in [1, 64]");
        std::vector<std::pair<int, int>> w(nslots);
        for (int b = 0; b < nslots; ++b) {
            MI_REQUIRE(hist[b] >= 0 && hist[b] <= max_seq, who + ": hist must be in [0, max_seq]");
            w[b] = {hist[b], 0};
        }
        u.inputs(qkv, nslots, kc, vc, nslots, mem);
        u.state(w);
        launch_gpt_attn1(dtype, u.q.p, u.k.p, u.v.p, u.o.p, u.st.as<int>(), heads, nslots, u.hidden, max_seq, 1, u.slot_elems(), u.s);
        u.result(out, nslots, mem);
    });
}

int mi_gpt_attn_decode_beam(const float* qkv, const float* kc, const float* vc, int dtype, int heads, int max_seq, int nslots,
                            const int32_t* hist, const int32_t* ndec, int beams, const int32_t* anc, float* out, int mem) {
    return guard([&] {
        const std::string who = "mi_gpt_attn_decode_beam";
        AttnUnit u(who, dtype, heads, max_seq, mem);
        MI_REQUIRE(qkv && kc && vc && hist && ndec && anc && out, who + ": null argument");
        MI_REQUIRE(nslots >= 1 && nslots <= GPT_MAX_BATCH, who + ": nslots must be in [1, 64]");
        MI_REQUIRE(beams >= 1 && beams <= GPT_BEAM_MAX && nslots % beams == 0, who + ": beams must be in [1, 8] and divide nslots");
        std::vector<std::pair<int, int>> w(nslots);
        for (int b = 0; b < nslots; ++b) {
            MI_REQUIRE(hist[b] >= 0 && hist[b] <= max_seq, who + ": hist must be in [0, max_seq]");
            MI_REQUIRE(ndec[b] >= 0 && ndec[b] <= hist[b] + 1, who + ": ndec must be in [0, hist + 1]");
            w[b] = {hist[b], ndec[b]};
        }
        const size_t na = (size_t)2 * nslots * max_seq;
        for (size_t i = 0; i < na; ++i) MI_REQUIRE(anc[i] >= 0 && anc[i] < beams, who + ": ancestor table entries must be in [0, beams)");
        u.inputs(qkv, nslots, kc, vc, nslots, mem);
        u.state(w);
        DevBuf tab;
        tab.ensure(na * 4);
        MI_HIP(hipMemcpyAsync(tab.p, anc, na * 4, hipMemcpyHostToDevice, u.s));
        launch_gpt_attn1_beam(dtype, u.q.p, u.k.p, u.v.p, u.o.p, u.st.as<int>(), tab.as<int>(), tab.as<int>() + (size_t)nslots * max_seq,
                              heads, nslots, u.hidden, max_seq, u.slot_elems(), beams, u.s);
        u.result(out, nslots, mem);
    });
}

int mi_gpt_attn_prompt(const float* qkv, const float* kc, const float* vc, int dtype, int heads, int max_seq, int hist, int rows,
                       int flag, float* out, int mem) {
    return guard([&] {
        const std::string who = "mi_gpt_attn_prompt";
        AttnUnit u(who, dtype, heads, max_seq, mem);
        MI_REQUIRE(qkv && kc && vc && out, who + ": null argument");
        MI_REQUIRE(hist >= 0 && rows >= 1 && hist + rows <= max_seq, who + ": hist + rows exceeds max_seq");
        MI_REQUIRE(flag == 0 || flag == 1, who + ": flag must be 0 or 1");
        u.inputs(qkv, rows, kc, vc, 1, mem);
        u.state({{hist, 0}});
        launch_gpt_attn_prompt(dtype, u.q.p, u.k.p, u.v.p, u.o.p, u.st.as<int>(), heads, rows, flag, u.hidden, max_seq, u.s);
        u.result(out, rows, mem);
    });
}

int mi_gpt_attn_prompt_packed(const float* qkv, const float* kc, const float* vc, int dtype, int heads, int max_seq, int nslots,
                              const int32_t* segs, int nseg, int total, float* out, int mem) {
    return guard([&] {
        const std::string who = "mi_gpt_attn_prompt_packed";
        AttnUnit u(who, dtype, heads, max_seq, mem);
        MI_REQUIRE(qkv && kc && vc && segs && out, who + ": null argument");
        MI_REQUIRE(nslots >= 1 && nslots <= GPT_MAX_BATCH && nseg >= 1 && nseg <= nslots, who + ": nslots must be in [1, 64], nseg in [1, nslots]");
        std::vector<Gpt::Seg> tab(nseg);
        int sum = 0;
        uint64_t used = 0;
        for (int g = 0; g < nseg; ++g) {
            const int32_t first = segs[3 * g], rows = segs[3 * g + 1], slot = segs[3 * g + 2];
            MI_REQUIRE(first == sum && rows >= 1 && rows <= max_seq - sum, who + ": segments must be ascending and gap-free within max_seq");
            MI_REQUIRE(slot >= 0 && slot < nslots && !(used >> slot & 1u), who + ": segment slot out of range or used twice");
            used |= (uint64_t)1 << slot;
            sum += rows;
            tab[g] = {first, rows, slot, 0};
        }
        MI_REQUIRE(sum == total, who + ": total must be the sum of the segments' rows");
        u.inputs(qkv, total, kc, vc, nslots, mem);
        DevBuf dtab;
        dtab.ensure(tab.size() * sizeof(Gpt::Seg));
        MI_HIP(hipMemcpyAsync(dtab.p, tab.data(), tab.size() * sizeof(Gpt::Seg), hipMemcpyHostToDevice, u.s));
        launch_gpt_attn_packed(dtype, u.q.p, u.k.p, u.v.p, u.o.p, dtab.p, nseg, total, heads, u.hidden, max_seq, nslots, u.slot_elems(), u.s);
        u.result(out, total, mem);
    });
}

int mi_gpt_linear_batch_rows(int nb) { return nb >= 1 && nb <= GPT_MAX_BATCH ? gpt_padded_rows(nb) : MI_EINVAL; }

// uint8 weights of a unit entry: null q = the fp32 matrix w, rounded to dtype
struct LinQ8 { const uint8_t* q; const float* scale; const uint8_t* zp; };

// the weights of a unit entry on the device, as the launchers take them
static GptLin lin_unit_weights(LinUnit& u, const std::string& who, const float* w, const LinQ8& q8, const float* bias, int dtype,
                               int n, int k) {
    if (!q8.q) {
        MI_REQUIRE(w, who + ": null argument");
        MI_REQUIRE(k % 8 == 0, who + ": k must be a multiple of 8");
        return GptLin{dtype, u.typed(w, n, k, dtype), u.f32(bias, n), n, k};
    }
    MI_REQUIRE(q8.scale && q8.zp, who + ": null argument");
    MI_REQUIRE(dtype == MI_F16, who + ": uint8 weights run with MI_F16 activations");
    MI_REQUIRE(k % 16 == 0, who + ": k must be a multiple of 16");
    return GptLin{dtype, u.bytes(q8.q, (size_t)n * k), u.f32(bias, n), n, k, GPT_W_Q8, u.f32(q8.scale, n), (const uint8_t*)u.bytes(q8.zp, n)};
}

static int linear_decode_unit(const std::string& who, const float* w, const LinQ8& q8, const float* bias, const float* x, int dtype,
                              int n, int k, const float* ln_w, const float* ln_b, const float* pre_w, const float* pre_b,
                              float* pre_out, const float* res, int act, int out_f32, int qkv, int hist, int max_seq, float* kc,
                              float* vc, float* out, int mem) {
    return guard([&] {
        LinUnit u(who, dtype, mem);
        MI_REQUIRE(x && out, who + ": null argument");
        MI_REQUIRE(n >= 1 && n <= (1 << 20) && k >= 1 && k <= 16384, who + ": n must be in [1, 2^20], k in [1, 16384]");
        MI_REQUIRE(!ln_w == !ln_b && !pre_w == !pre_b, who + ": a LayerNorm needs both its vectors");
        MI_REQUIRE(act == ACT_NONE || act == ACT_GELU_TANH, who + ": act must be 0 or 1 (gelu_new)");
        if (qkv) {
            MI_REQUIRE(n % 3 == 0 && n == 3 * k && k % 64 == 0, who + ": qkv needs n == 3 * k (a multiple of 3), k a multiple of 64");
            MI_REQUIRE(kc && vc, who + ": qkv needs kc and vc");
            MI_REQUIRE(max_seq >= 1 && max_seq <= 8192 && hist >= 0 && hist <= max_seq, who + ": 0 <= hist <= max_seq <= 8192");
        }
        const int odt = out_f32 ? MI_F32 : dtype;
        const size_t nc = qkv ? (size_t)k * max_seq : 0;
        const GptLin l = lin_unit_weights(u, who, w, q8, bias, dtype, n, k);
        const void* xd = ln_w ? (const void*)u.f32(x, k) : u.typed(x, 1, k, dtype);
        void* kd = qkv ? u.typed(kc, (long)(nc / 64), 64, dtype) : nullptr;
        void* vd = qkv ? u.typed(vc, (long)(nc / 64), 64, dtype) : nullptr;
        void* od = u.nan_out(n, odt);
        float* pd = pre_w ? (float*)u.nan_out(k, MI_F32) : nullptr;
        const int* st = u.state(&hist, 1, 1);
        launch_gpt_gemv(l, xd, u.f32(ln_w, k), u.f32(ln_b, k), u.f32(pre_w, k), u.f32(pre_b, k), pd, od, odt, act, u.f32(res, n), kd,
                        vd, st, qkv ? max_seq : 1, u.s);
        u.give(out, od, n, odt);
        if (pd) u.give(pre_out, pd, k, MI_F32);
        if (qkv) { u.give(kc, kd, nc, dtype); u.give(vc, vd, nc, dtype); }
        MI_HIP(hipStreamSynchronize(u.s));
    });
}

int mi_gpt_linear_decode(const float* w, const float* bias, const float* x, int dtype, int n, int k, const float* ln_w,
                         const float* ln_b, const float* pre_w, const float* pre_b, float* pre_out, const float* res, int act,
                         int out_f32, int qkv, int hist, int max_seq, float* kc, float* vc, float* out, int mem) {
    return linear_decode_unit("mi_gpt_linear_decode", w, LinQ8{nullptr, nullptr, nullptr}, bias, x, dtype, n, k, ln_w, ln_b, pre_w, pre_b,
                              pre_out, res, act, out_f32, qkv, hist, max_seq, kc, vc, out, mem);
}

int mi_gpt_linear_decode_q8(const uint8_t* q, const float* scale, const uint8_t* zp, const float* bias, const float* x, int dtype, int n,
                            int k, const float* ln_w, const float* ln_b, const float* pre_w, const float* pre_b, float* pre_out,
                            const float* res, int act, int out_f32, int qkv, int hist, int max_seq, float* kc, float* vc, float* out,
                            int mem) {
    if (!q) return guard([&] { MI_REQUIRE(false, "mi_gpt_linear_decode_q8: null argument"); });
    return linear_decode_unit("mi_gpt_linear_decode_q8", nullptr, LinQ8{q, scale, zp}, bias, x, dtype, n, k, ln_w, ln_b, pre_w, pre_b,
                              pre_out, res, act, out_f32, qkv, hist, max_seq, kc, vc, out, mem);
}

static int linear_batch_unit(const std::string& who, const float* w, const LinQ8& q8, const float* bias, const float* x,
                             const float* x_dead, int dtype, int n, int k, int nb, const float* res, int act, int out_f32, int qkv,
                             const int32_t* hist, int max_seq, float* kc, float* vc, float* out, int mem) {
    return guard([&] {
        LinUnit u(who, dtype, mem);
        MI_REQUIRE(x && out, who + ": null argument");
        MI_REQUIRE(nb >= 1 && nb <= GPT_MAX_BATCH, who + ": nb must be in [1, 64]");
        MI_REQUIRE(n >= 1 && n <= (1 << 20) && k >= 1 && k <= 16384, who + ": n must be in [1, 2^20], k in [1, 16384]");
        MI_REQUIRE(act == ACT_NONE || act == ACT_GELU_TANH, who + ": act must be 0 or 1 (gelu_new)");
        if (qkv) {
            MI_REQUIRE(n % 3 == 0 && n == 3 * k && k % 64 == 0, who + ": qkv needs n == 3 * k (a multiple of 3), k a multiple of 64");
            MI_REQUIRE(kc && vc && hist, who + ": qkv needs kc, vc and hist");
            MI_REQUIRE(max_seq >= 1 && max_seq <= 8192, who + ": max_seq must be in [1, 8192]");
            for (int b = 0; b < nb; ++b) MI_REQUIRE(hist[b] >= 0 && hist[b] <= max_seq, who + ": hist must be in [0, max_seq]");
        }
        const int odt = out_f32 ? MI_F32 : dtype, P = gpt_padded_rows(nb);
        const size_t sstride = qkv ? (size_t)k * max_seq : 0, nc = (size_t)nb * sstride;
        const GptLin l = lin_unit_weights(u, who, w, q8, bias, dtype, n, k);
        char* xd = (char*)u.typed(x, nb, k, dtype, P);
        const size_t row = (size_t)k * dtype_size(dtype);
        if (x_dead) {
            const float* dead = u.f32(x_dead, k);
            for (int b = nb; b < P; ++b) launch_copy2d(dead, k, xd + b * row, k, 1, k, dtype, u.s);
        } else if (P > nb) {
            MI_HIP(hipMemsetAsync(xd + nb * row, 0, (P - nb) * row, u.s));
        }
        void* kd = qkv ? u.typed(kc, (long)(nc / 64), 64, dtype) : nullptr;
        void* vd = qkv ? u.typed(vc, (long)(nc / 64), 64, dtype) : nullptr;
        void* od = u.nan_out((size_t)P * n, odt);
        const int* st = u.state(qkv ? hist : nullptr, nb, P);
        launch_gpt_gemv_b(l, xd, nb, P, od, odt, act, u.f32(res, (size_t)nb * n), kd, vd, st, qkv ? max_seq : 1, sstride, u.s);
        u.give(out, od, (size_t)P * n, odt);
        if (qkv) { u.give(kc, kd, nc, dtype); u.give(vc, vd, nc, dtype); }
        MI_HIP(hipStreamSynchronize(u.s));
    });
}

int mi_gpt_linear_batch(const float* w, const float* bias, const float* x, const float* x_dead, int dtype, int n, int k, int nb,
                        const float* res, int act, int out_f32, int qkv, const int32_t* hist, int max_seq, float* kc, float* vc,
                        float* out, int mem) {
    return linear_batch_unit("mi_gpt_linear_batch", w, LinQ8{nullptr, nullptr, nullptr}, bias, x, x_dead, dtype, n, k, nb, res, act, out_f32,
                             qkv, hist, max_seq, kc, vc, out, mem);
}

int mi_gpt_linear_batch_q8(const uint8_t* q, const float* scale, const uint8_t* zp, const float* bias, const float* x,
                           const float* x_dead, int dtype, int n, int k, int nb, const float* res, int act, int out_f32, int qkv,
                           const int32_t* hist, int max_seq, float* kc, float* vc, float* out, int mem) {
    if (!q) return guard([&] { MI_REQUIRE(false, "mi_gpt_linear_batch_q8: null argument"); });
    return linear_batch_unit("mi_gpt_linear_batch_q8", nullptr, LinQ8{q, scale, zp}, bias, x, x_dead, dtype, n, k, nb, res, act, out_f32,
                             qkv, hist, max_seq, kc, vc, out, mem);
}

// The ConvGemm of mi_bench_conv_gemm's arguments, its operands from buf(which, bytes): device memory to launch it, aligned dummies
// that nobody dereferences to plan it (mi_conv_gemm_plan).  Decides which operands exist: the weight planes w3 (bf16x3 kernel), the
// panel planes xp / w3p (gemm_x3p.hip), the stream-K workspace of 1024 slots.
extern "C++" {
enum { BG_X, BG_W, BG_BIAS, BG_OUT, BG_RES, BG_W3, BG_XP, BG_W3P, BG_SK_WS, BG_SK_FLAGS, BG_COUNT };
template <typename F> static ConvGemm bench_gemm(int dtype, int B, int T, int Cin, int N, int taps, int dil, int with_res, F&& buf) {
    const size_t es = dtype_size(dtype), nx = (size_t)B * T * Cin, nw = (size_t)N * taps * Cin, no = (size_t)B * T * N;
    ConvGemm p;
    p.dtype = dtype; p.x = buf(BG_X, nx * es); p.w = buf(BG_W, nw * es); p.bias = (const float*)buf(BG_BIAS, (size_t)N * 4); p.out = buf(BG_OUT, no * es);
    p.res = with_res ? buf(BG_RES, no * es) : nullptr;
    p.B = B; p.T_in = T; p.M = T; p.N = N; p.Cin = Cin; p.taps = taps; p.dil = dil; p.pad = (taps * dil - dil) / 2;
    p.x_bstride = (long)T * Cin; p.x_rstride = Cin; p.out_bstride = (long)T * N; p.out_rstride = N;
    p.sk_slots = 1024; p.sk_ws = (float*)buf(BG_SK_WS, (size_t)p.sk_slots * 128 * 128 * 4); p.sk_flags = (int*)buf(BG_SK_FLAGS, (size_t)p.sk_slots * 4);
    if (dtype == MI_F32 && taps == 1 && gemm_x3_enabled()) p.w3 = buf(BG_W3, (size_t)3 * nw * 2);      // the bf16x3 kernel needs the weight planes
    if (p.w3 && gemm_x3p_enabled() && N % 128 == 0 && Cin % 32 == 0 && p.pad == 0) {       // ... and the panel-plane form (gemm_x3p.hip)
        p.np = x3p_planes();
        p.xp = buf(BG_XP, (size_t)x3p_bytes((long)B * T, Cin, p.np)); p.w3p = buf(BG_W3P, (size_t)x3p_bytes(N, Cin, p.np));
    }
    return p;
}
}  // extern "C++"

int mi_conv_gemm_plan(int dtype, int B, int T, int Cin, int N, int taps, int dil, int with_res, int cus, int32_t* plans, int* n_launches) {
    return guard([&] {
        MI_REQUIRE(plans && n_launches && (dtype == MI_F32 || dtype == MI_F16 || dtype == MI_BF16) && B > 0 && T > 0 && Cin > 0 && N > 0 && taps > 0 && dil > 0 && cus > 0,
                   "mi_conv_gemm_plan: bad arguments");
        ConvGemm p = bench_gemm(dtype, B, T, Cin, N, taps, dil, with_res, [](int which, size_t) { return (void*)(uintptr_t)(4096 * (which + 1)); });
        gemm_one_m_axis(p);
        int n = 0;
        for (;;) {
            const GemmPlan g = gemm_plan(p, cus);
            const int32_t row[MI_GEMM_PLAN_INTS] = {g.kind, g.Tm, g.Tn, g.RT, g.RC, g.lds_epi, g.use_buf, (int32_t)g.grid[0], (int32_t)g.grid[1], (int32_t)g.grid[2]};
            std::memcpy(plans + (size_t)n++ * MI_GEMM_PLAN_INTS, row, sizeof(row));
            if (!g.split_rows || n == 2) break;
            p.M = p.T_in = p.M - g.split_rows;        // the rest of a row split is a problem of its own (pointers: nobody reads them here)
        }
        *n_launches = n;
    });
}

int mi_bench_conv_gemm(int dtype, int B, int T, int Cin, int N, int taps, int dil, int with_res, int iters, double* ms) {
    return guard([&] {
        MI_REQUIRE(ms && B > 0 && T > 0 && Cin > 0 && N > 0 && taps > 0 && iters > 0, "mi_bench_conv_gemm: bad arguments");
        hipStream_t s;
        MI_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        const size_t es = dtype_size(dtype);
        const size_t nx = (size_t)B * T * Cin, nw = (size_t)N * taps * Cin, no = (size_t)B * T * N;
        DevBuf bufs[BG_COUNT];
        SkWorkspace skw;
        ConvGemm p = bench_gemm(dtype, B, T, Cin, N, taps, dil, with_res, [&](int which, size_t bytes) -> void* {
            if (which == BG_SK_WS || which == BG_SK_FLAGS) { skw.ensure(1024, s); return which == BG_SK_WS ? skw.ws.p : skw.flags.p; }
            bufs[which].ensure(bytes);
            return bufs[which].p;
        });
        DevBuf &x = bufs[BG_X], &w = bufs[BG_W], &w3p = bufs[BG_W3P];
        std::vector<float> hx(nx), hw(nw), hb(N, 0.01f);
        uint32_t st = 12345;
        auto rnd = [&]() { st = st * 1664525u + 1013904223u; return ((st >> 8) & 0xffff) / 65536.0f - 0.5f; };
        for (auto& v : hx) v = rnd();
        for (auto& v : hw) v = rnd() * 0.1f;
        if (env_first_is("MI355TTS_BENCH_ZERO", '1')) { std::fill(hx.begin(), hx.end(), 0.f); std::fill(hw.begin(), hw.end(), 0.f); }   // data-dependent power / clock check
        // MI355TTS_BENCH_WSETS=n: cycle through n copies of the weights (n * bytes > 256 MiB MALL => every launch
        // streams cold weights from HBM, like consecutive layers of a real model)
        const int nsets = std::max(1, (int)env_int("MI355TTS_BENCH_WSETS", 1));
        upload_as(x, hx.data(), nx, dtype, s); upload_as(w, hw.data(), nw, dtype, s); upload_f32(bufs[BG_BIAS], hb.data(), N, s);
        DevBuf wsets;
        if (nsets > 1) {
            wsets.ensure((size_t)nsets * nw * es);
            for (int i = 0; i < nsets; ++i)
                MI_HIP(hipMemcpyAsync((char*)wsets.p + (size_t)i * nw * es, w.p, nw * es, hipMemcpyDeviceToDevice, s));
        }
        if (p.res) MI_HIP(hipMemsetAsync(bufs[BG_RES].p, 0, no * es, s));
        if (p.w3) split3_planes((const float*)w.p, bufs[BG_W3].p, (long)nw, s);
        if (p.xp) {
            x3p_split_rows((const float*)x.p, Cin, bufs[BG_XP].p, B * T, Cin, s, p.np);
            x3p_split_rows((const float*)w.p, Cin, w3p.p, N, Cin, s, p.np);
        }
        // panel-plane launches with MI355TTS_BENCH_WSETS: n copies of the weight PLANES (the kernel never reads p.w)
        DevBuf w3psets;
        const size_t w3pb = p.w3p ? (size_t)x3p_bytes(N, Cin, p.np) : 0;
        if (nsets > 1 && p.w3p) {
            w3psets.ensure((size_t)nsets * w3pb);
            for (int i = 0; i < nsets; ++i) MI_HIP(hipMemcpyAsync((char*)w3psets.p + (size_t)i * w3pb, w3p.p, w3pb, hipMemcpyDeviceToDevice, s));
        }
        for (int i = 0; i < 3; ++i) launch_conv_gemm(p, s);
        hipEvent_t e0, e1;
        MI_HIP(hipEventCreate(&e0)); MI_HIP(hipEventCreate(&e1));
        MI_HIP(hipEventRecord(e0, s));
        for (int i = 0; i < iters; ++i) {
            if (nsets > 1) p.w = (char*)wsets.p + (size_t)(i % nsets) * nw * es;
            if (nsets > 1 && p.w3p) p.w3p = (char*)w3psets.p + (size_t)(i % nsets) * w3pb;
            launch_conv_gemm(p, s);
        }
        MI_HIP(hipEventRecord(e1, s));
        MI_HIP(hipEventSynchronize(e1));
        float t = 0.f;
        MI_HIP(hipEventElapsedTime(&t, e0, e1));
        *ms = (double)t / iters;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipStreamDestroy(s);
    });
}

// ---------------------------------------------------------------------------------------------------------------
// IndexTTS graph A (cond.hip)
// ---------------------------------------------------------------------------------------------------------------
int64_t mi_indextts_cond_param_count(const int32_t* cfg, int n_cfg) {
    int64_t n = -1;
    int rc = guard([&] { n = cond_param_count(parse_cond_cfg(cfg, n_cfg)); });
    return rc == MI_OK ? n : (int64_t)rc;
}

mi_cond* mi_indextts_cond_create(const int32_t* cfg, int n_cfg, const float* weights, int64_t n_weights, int device) {
    mi_cond* h = nullptr;
    int rc = guard([&] {
        MI_REQUIRE(weights != nullptr, "mi_indextts_cond_create: null weights");
        Cond* impl = cond_create(parse_cond_cfg(cfg, n_cfg), weights, n_weights, device);
        h = new mi_cond; h->impl = impl;
    });
    return rc == MI_OK ? h : nullptr;
}

void mi_indextts_cond_destroy(mi_cond* h) {
    if (!h) return;
    cond_destroy(h->impl);
    delete h;
}

int mi_indextts_cond_run(mi_cond* h, const int16_t* audio, int64_t L, float* conds, float* conds_latent, float* mel, int mem) {
    return guard([&] {
        MI_REQUIRE(h && h->impl, "mi_indextts_cond_run: null handle");
        std::lock_guard<std::mutex> lk_(h->mu);
        MI_REQUIRE(mem == MI_HOST || mem == MI_DEVICE, "mi_indextts_cond_run: bad mem kind");
        cond_run(h->impl, audio, (long)L, conds, conds_latent, mel, mem);
    });
}

int mi_set_option(const char* key, int64_t value) {
    return guard([&] {
        MI_REQUIRE(key != nullptr, "mi_set_option: null key");
        if (!options_set(key, (long)value)) throw Error(MI_EINVAL, std::string("mi_set_option: unknown key ") + key);
        option_epoch_bump();
    }, /*exclusive=*/true);
}

int mi_get_option(const char* key, int64_t* value) {
    return guard([&] {
        MI_REQUIRE(key != nullptr && value != nullptr, "mi_get_option: null key or value");
        long v = 0;
        if (!options_get(key, &v)) throw Error(MI_EINVAL, std::string("mi_get_option: unknown key ") + key);
        *value = v;
    });
}

int mi_device_pci_bus_id(int device, char* buf, int cap) {
    return guard([&] {
        MI_REQUIRE(buf && cap >= 16, "mi_device_pci_bus_id: buffer of at least 16 bytes");
        MI_HIP(hipDeviceGetPCIBusId(buf, cap, device));
    });
}

int mi_prof_enable(int family_mask) { prof_enable((unsigned)family_mask); return MI_OK; }
int mi_prof_reset(void) { return guard([&] { prof_reset(); }); }
int mi_prof_kernel_count(void) { return prof_kernel_count(); }
int mi_prof_kernel_get(int index, char* name, int name_cap, char* family, int family_cap, double* ms, int64_t* launches,
                       double* bytes, double* flops) {
    return guard([&] {
        std::string n;
        int f = 0;
        double m = 0, b = 0, fl = 0;
        int64_t l = 0;
        MI_REQUIRE(name && name_cap > 1 && prof_kernel_get(index, &n, &f, &m, &l, &b, &fl), "mi_prof_kernel_get: bad index");
        std::snprintf(name, (size_t)name_cap, "%s", n.c_str());
        static const char* fams[] = {"conv_gemm", "aa_act", "conv_post", "attn", "norm", "other"};
        if (family && family_cap > 1) std::snprintf(family, (size_t)family_cap, "%s", fams[f]);
        if (ms) *ms = m;
        if (launches) *launches = l;
        if (bytes) *bytes = b;
        if (flops) *flops = fl;
    });
}
int mi_prof_get(const char* family, double* ms, int64_t* launches, double* bytes, double* flops) {
    return guard([&] {
        MI_REQUIRE(family != nullptr, "mi_prof_get: null family");
        const int f = prof_family(family);
        MI_REQUIRE(f >= 0, "mi_prof_get: unknown kernel family");
        prof_get(f, ms, launches, bytes, flops);
    });
}

}  // extern "C"
