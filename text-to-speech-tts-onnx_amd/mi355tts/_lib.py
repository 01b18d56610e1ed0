"""ctypes binding of libmi355tts.so (C-ABI: include/mi355tts.h).

The product path has NO CPU fallback: if the shared library is missing or no MI355X is visible,
calls raise loudly.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

MI_F32, MI_F16, MI_BF16 = 0, 1, 2
MI_HOST, MI_DEVICE = 0, 1
MI_EINVAL = -1
MI_ESTATE = -4
DTYPES = {"f32": MI_F32, "fp32": MI_F32, "float32": MI_F32, "f16": MI_F16, "fp16": MI_F16, "float16": MI_F16,
          "bf16": MI_BF16, "bfloat16": MI_BF16}

# MI355TTS_LIB: another build of the same library (A/B measurements of kernel variants); the default is the in-tree build
_LIB_PATH = os.environ.get("MI355TTS_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libmi355tts.so")
_lib = None


class MiError(RuntimeError):
    pass


def lib_path() -> str:
    return _LIB_PATH


def load() -> C.CDLL:
    """dlopen the engine (no GPU needed for this step) and declare every prototype."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise MiError(f"{_LIB_PATH} is missing: build it with `python text-to-speech-tts-onnx_amd/build.py` "
                      f"(or __graft_entry__.build()); there is no CPU fallback")
    # torch-ROCm ships its own copy of the HIP runtime.  If this library's copy initialises first, a later
    # `torch.cuda` initialisation in the same process reports "No HIP GPUs are available" (seen with the device-resident
    # OrtValues of ort_compat in a script that opened its sessions before touching torch); the other order works.  So when
    # torch is installed it goes first (MI355TTS_NO_TORCH=1 skips this for pure-numpy users who never hand over torch tensors).
    # A torch install that cannot even be imported (missing, or broken: OSError / RuntimeError from a mismatched build) must not
    # make THIS library unloadable: numpy-only callers never need it.
    if os.environ.get("MI355TTS_NO_TORCH") != "1":
        try:
            import torch
            torch.cuda.is_available()
        except Exception:
            pass
    L = C.CDLL(_LIB_PATH)
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    vp = C.c_void_p
    L.mi_init.argtypes = [C.c_int]; L.mi_init.restype = C.c_int
    L.mi_device_count.argtypes = []; L.mi_device_count.restype = C.c_int
    L.mi_last_error.argtypes = []; L.mi_last_error.restype = C.c_char_p
    L.mi_version.argtypes = []; L.mi_version.restype = C.c_char_p
    L.mi_bigvgan_param_count.argtypes = [i32p, C.c_int]; L.mi_bigvgan_param_count.restype = C.c_int64
    L.mi_bigvgan_create.argtypes = [i32p, C.c_int, f32p, C.c_int64, C.c_int, C.c_int]
    L.mi_bigvgan_create.restype = vp
    L.mi_bigvgan_create_mem.argtypes = [i32p, C.c_int, vp, C.c_int64, C.c_int, C.c_int, C.c_int]
    L.mi_bigvgan_create_mem.restype = vp
    L.mi_bigvgan_destroy.argtypes = [vp]; L.mi_bigvgan_destroy.restype = None
    L.mi_bigvgan_out_len.argtypes = [vp, C.c_int]; L.mi_bigvgan_out_len.restype = C.c_int64
    L.mi_bigvgan_forward.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int]; L.mi_bigvgan_forward.restype = C.c_int
    L.mi_bigvgan_forward_f32.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int]
    L.mi_bigvgan_forward_f32.restype = C.c_int
    L.mi_bigvgan_forward_latent.argtypes = [vp, vp, C.c_int, vp, C.c_int64, vp, vp, C.c_int]
    L.mi_bigvgan_forward_latent.restype = C.c_int
    L.mi_aa_activation1d.argtypes = [f32p, C.c_int, C.c_int, C.c_int, f32p, f32p, C.c_int, C.c_int, C.c_int, f32p]
    L.mi_aa_activation1d.restype = C.c_int
    L.mi_aa_conv1d.argtypes = [f32p, C.c_int, C.c_int, C.c_int, f32p, f32p, C.c_int, f32p, f32p, C.c_int, C.c_int, f32p, C.c_int, f32p]
    L.mi_aa_conv1d.restype = C.c_int
    L.mi_conv1d.argtypes = [f32p, C.c_int, C.c_int, C.c_int, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                            C.c_int, f32p]
    L.mi_conv1d.restype = C.c_int
    L.mi_conv_transpose1d.argtypes = [f32p, C.c_int, C.c_int, C.c_int, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, f32p]
    L.mi_conv_transpose1d.restype = C.c_int
    i16p, i64p = C.POINTER(C.c_int16), C.POINTER(C.c_int64)
    L.mi_f5_param_count.argtypes = [i32p, C.c_int, f32p, C.c_int]; L.mi_f5_param_count.restype = C.c_int64
    L.mi_f5_create.argtypes = [i32p, C.c_int, f32p, C.c_int, f32p, C.c_int64, C.c_int, C.c_int]
    L.mi_f5_create.restype = vp
    L.mi_f5_create_mem.argtypes = [i32p, C.c_int, f32p, C.c_int, vp, C.c_int64, C.c_int, C.c_int, C.c_int]
    L.mi_f5_create_mem.restype = vp
    L.mi_f5_destroy.argtypes = [vp]; L.mi_f5_destroy.restype = None
    L.mi_f5_tables.argtypes = [vp, f32p, f32p]; L.mi_f5_tables.restype = C.c_int
    L.mi_f5_info.argtypes = [vp, C.c_char_p]; L.mi_f5_info.restype = C.c_int64
    L.mi_f5_preprocess.argtypes = [vp, vp, C.c_int64, vp, C.c_int64, C.c_int64, vp, C.c_uint64, vp, vp, vp, vp, vp,
                                   i64p, C.c_int]
    L.mi_f5_preprocess.restype = C.c_int
    L.mi_f5_stft.argtypes = [vp, vp, C.c_int64, vp, C.c_int]; L.mi_f5_stft.restype = C.c_int
    L.mi_f5_transformer_step.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int64, i32p, C.c_int, C.c_int]
    L.mi_f5_transformer_step.restype = C.c_int
    L.mi_f5_sample.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int]
    L.mi_f5_sample.restype = C.c_int
    L.mi_f5_dit_eval.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int64, C.c_int, vp, C.c_int]
    L.mi_f5_dit_eval.restype = C.c_int
    L.mi_f5_decode.argtypes = [vp, vp, C.c_int, C.c_int64, C.c_int64, vp, vp, i64p, C.c_int]
    L.mi_f5_decode.restype = C.c_int
    L.mi_f5_synthesize.argtypes = [vp, C.c_int, vp, C.c_int64, vp, C.c_int64, C.c_int64, vp, C.c_uint64, vp, i64p,
                                   C.c_int]
    L.mi_f5_synthesize.restype = C.c_int
    L.mi_f5_synthesize_mel.argtypes = [vp, C.c_int, vp, C.c_int64, vp, C.c_int64, C.c_int64, vp, C.c_uint64, vp, i64p,
                                       C.c_int]
    L.mi_f5_synthesize_mel.restype = C.c_int
    L.mi_f5_synthesize_ragged.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_uint64, vp, C.c_int64, vp, C.c_int]
    L.mi_f5_synthesize_ragged.restype = C.c_int
    L.mi_f5_dit_eval_ragged.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int64, C.c_int, vp, C.c_int]
    L.mi_f5_dit_eval_ragged.restype = C.c_int
    L.mi_f5_synthesize_mel_ragged.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_uint64, vp, C.c_int64, vp, C.c_int]
    L.mi_f5_synthesize_mel_ragged.restype = C.c_int
    L.mi_bigvgan_forward_ragged.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int64, vp, C.c_int]
    L.mi_bigvgan_forward_ragged.restype = C.c_int
    L.mi_bigvgan_forward_latent_ragged.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int64, vp, vp, C.c_int64, vp, C.c_int]
    L.mi_bigvgan_forward_latent_ragged.restype = C.c_int
    if hasattr(L, "mi_bigvgan_forward_latent_voices"):       # absent from an older build loaded through MI355TTS_LIB (A/B runs)
        L.mi_bigvgan_forward_latent_voices.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, C.c_int64, vp, vp, vp, C.c_int64, vp, C.c_int]
        L.mi_bigvgan_forward_latent_voices.restype = C.c_int
    if hasattr(L, "mi_bigvgan_forward_latent_windows"):
        L.mi_bigvgan_forward_latent_windows.argtypes = [vp, C.c_int, vp, C.c_int64, vp, vp, vp, vp, C.c_int, vp, C.c_int64, vp, vp, vp,
                                                        C.c_int64, vp, C.c_int]
        L.mi_bigvgan_forward_latent_windows.restype = C.c_int
    L.mi_indextts_cond_param_count.argtypes = [C.POINTER(C.c_int32), C.c_int]; L.mi_indextts_cond_param_count.restype = C.c_int64
    L.mi_indextts_cond_create.argtypes = [C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_float), C.c_int64, C.c_int]
    L.mi_indextts_cond_create.restype = vp
    L.mi_indextts_cond_destroy.argtypes = [vp]; L.mi_indextts_cond_destroy.restype = None
    L.mi_indextts_cond_run.argtypes = [vp, vp, C.c_int64, vp, vp, vp, C.c_int]; L.mi_indextts_cond_run.restype = C.c_int
    L.mi_gpt_param_count.argtypes = [C.POINTER(C.c_int32), C.c_int]; L.mi_gpt_param_count.restype = C.c_int64
    L.mi_gpt_create.argtypes = [C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_float), C.c_int64, C.c_int, C.c_int]
    L.mi_gpt_create.restype = C.c_void_p
    L.mi_gpt_create_mem.argtypes = [C.POINTER(C.c_int32), C.c_int, vp, C.c_int64, C.c_int, C.c_int, C.c_int]
    L.mi_gpt_create_mem.restype = C.c_void_p
    L.mi_gpt_destroy.argtypes = [vp]; L.mi_gpt_destroy.restype = None
    L.mi_gpt_text_embed.argtypes = [vp, vp, C.c_int, vp, C.c_int]; L.mi_gpt_text_embed.restype = C.c_int
    L.mi_gpt_mel_embed.argtypes = [vp, C.c_int32, C.c_int64, vp, C.c_int]; L.mi_gpt_mel_embed.restype = C.c_int
    L.mi_gpt_reset.argtypes = [vp]; L.mi_gpt_reset.restype = C.c_int
    L.mi_gpt_history_len.argtypes = [vp]; L.mi_gpt_history_len.restype = C.c_int64
    L.mi_gpt_step.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int]; L.mi_gpt_step.restype = C.c_int
    L.mi_gpt_kv_read.argtypes = [vp, C.c_int, vp, vp, C.c_int]; L.mi_gpt_kv_read.restype = C.c_int
    L.mi_gpt_kv_write.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int]; L.mi_gpt_kv_write.restype = C.c_int
    L.mi_gpt_generate.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_float, C.c_int, vp, vp, vp,
                                  C.POINTER(C.c_int32), C.c_int]
    L.mi_gpt_generate.restype = C.c_int
    L.mi_gpt_generate_batch.argtypes = [vp, C.c_int, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, C.c_int,
                                        C.c_float, C.c_int, vp, vp, vp, C.c_int, C.POINTER(C.c_int32), C.c_int]
    L.mi_gpt_generate_batch.restype = C.c_int
    L.mi_gpt_generate_sampled.argtypes = L.mi_gpt_generate.argtypes + [C.c_float, C.c_int, C.c_float, C.c_uint64]
    L.mi_gpt_generate_sampled.restype = C.c_int
    L.mi_gpt_generate_batch_sampled.argtypes = L.mi_gpt_generate_batch.argtypes + [vp, vp, vp, vp]
    L.mi_gpt_generate_batch_sampled.restype = C.c_int
    L.mi_gpt_generate_queue.argtypes = [vp, C.c_int, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, C.c_int, C.c_float,
                                        C.c_int, vp, vp, C.c_int, C.POINTER(C.c_int32), C.c_int, vp, vp, vp, vp, vp]
    L.mi_gpt_generate_queue.restype = C.c_int
    if hasattr(L, "mi_gpt_queue_begin"):
        L.mi_gpt_queue_begin.argtypes = [vp, C.c_int, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, C.c_int, C.c_float,
                                         C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]
        L.mi_gpt_queue_begin.restype = C.c_int
        L.mi_gpt_queue_advance.argtypes = [vp, vp, vp, vp, vp]; L.mi_gpt_queue_advance.restype = C.c_int
        L.mi_gpt_queue_end.argtypes = [vp]; L.mi_gpt_queue_end.restype = C.c_int
    if hasattr(L, "mi_gpt_generate_queue_beam"):
        L.mi_gpt_generate_queue_beam.argtypes = [vp, C.c_int, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, C.c_int,
                                                 C.c_float, C.c_int, C.c_int, vp, vp, C.c_int, C.POINTER(C.c_int32), vp, C.c_int, vp]
        L.mi_gpt_generate_queue_beam.restype = C.c_int
        L.mi_gpt_queue_begin_beam.argtypes = [vp, C.c_int, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, C.c_int, C.c_float,
                                              C.c_int, C.c_int, vp, vp, C.c_int, vp, C.c_int]
        L.mi_gpt_queue_begin_beam.restype = C.c_int
    if hasattr(L, "mi_gpt_generate_queue_beam_pool"):      # pool mode through the queue (absent from an older MI355TTS_LIB)
        L.mi_gpt_generate_queue_beam_pool.argtypes = [vp, C.c_int, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, C.c_int,
                                                      C.c_float, C.c_int, C.c_int, C.c_float, C.c_int, vp, vp, vp, vp, vp, vp,
                                                      C.c_int, C.POINTER(C.c_int32), vp, C.c_int, vp]
        L.mi_gpt_generate_queue_beam_pool.restype = C.c_int
        L.mi_gpt_queue_begin_beam_pool.argtypes = [vp, C.c_int, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, C.c_int,
                                                   C.c_float, C.c_int, C.c_int, C.c_float, C.c_int, vp, vp, vp, vp, vp, vp,
                                                   C.c_int, vp, C.c_int]
        L.mi_gpt_queue_begin_beam_pool.restype = C.c_int
    if hasattr(L, "mi_gpt_queue_schedule"):
        L.mi_gpt_queue_schedule.argtypes = [C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
        L.mi_gpt_queue_schedule.restype = C.c_int
    L.mi_gpt_sample_logits.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int]
    L.mi_gpt_sample_logits.restype = C.c_int
    L.mi_gpt_generate_beam.argtypes = [vp, C.c_int, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, C.c_int, C.c_float,
                                       C.c_int, vp, C.c_int, vp, vp, C.c_int, C.POINTER(C.c_int32), vp, C.c_int]
    L.mi_gpt_generate_beam.restype = C.c_int
    L.mi_gpt_beam_select.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int]
    L.mi_gpt_beam_select.restype = C.c_int
    if hasattr(L, "mi_gpt_generate_beam_pool"):
        L.mi_gpt_generate_beam_pool.argtypes = [vp, C.c_int, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, C.c_int, C.c_float,
                                                C.c_int, vp, C.c_int, C.c_float, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int,
                                                C.POINTER(C.c_int32), vp, C.c_int]
        L.mi_gpt_generate_beam_pool.restype = C.c_int
        L.mi_gpt_beam_pool_select.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, C.c_float,
                                              C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int]
        L.mi_gpt_beam_pool_select.restype = C.c_int
    if hasattr(L, "mi_gpt_attn_decode"):
        L.mi_gpt_attn_decode.argtypes = [vp, vp, vp] + [C.c_int] * 4 + [vp, vp, C.c_int]
        L.mi_gpt_attn_decode.restype = C.c_int
        L.mi_gpt_attn_decode_beam.argtypes = [vp, vp, vp] + [C.c_int] * 4 + [vp, vp, C.c_int, vp, vp, C.c_int]
        L.mi_gpt_attn_decode_beam.restype = C.c_int
        L.mi_gpt_attn_prompt.argtypes = [vp, vp, vp] + [C.c_int] * 6 + [vp, C.c_int]
        L.mi_gpt_attn_prompt.restype = C.c_int
        L.mi_gpt_attn_prompt_packed.argtypes = [vp, vp, vp] + [C.c_int] * 4 + [vp, C.c_int, C.c_int, vp, C.c_int]
        L.mi_gpt_attn_prompt_packed.restype = C.c_int
    if hasattr(L, "mi_gpt_linear_decode"):
        L.mi_gpt_linear_decode.argtypes = [vp, vp, vp] + [C.c_int] * 3 + [vp] * 6 + [C.c_int] * 5 + [vp, vp, vp, C.c_int]
        L.mi_gpt_linear_decode.restype = C.c_int
        L.mi_gpt_linear_batch.argtypes = [vp, vp, vp, vp] + [C.c_int] * 4 + [vp] + [C.c_int] * 3 + [vp, C.c_int, vp, vp, vp, C.c_int]
        L.mi_gpt_linear_batch.restype = C.c_int
        L.mi_gpt_linear_batch_rows.argtypes = [C.c_int]
        L.mi_gpt_linear_batch_rows.restype = C.c_int
    if hasattr(L, "mi_gpt_create_q8"):          # per-channel uint8 weights (csrc/gpt_q8.hip)
        L.mi_gpt_create_q8.argtypes = [C.POINTER(C.c_int32), C.c_int, vp, C.c_int64, C.c_int, C.c_int, C.c_int]
        L.mi_gpt_create_q8.restype = C.c_void_p
        L.mi_gpt_weight_bytes.argtypes = [vp]; L.mi_gpt_weight_bytes.restype = C.c_int64
        L.mi_gpt_quantize_u8.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp]; L.mi_gpt_quantize_u8.restype = C.c_int
        L.mi_gpt_linear_decode_q8.argtypes = [vp, vp] + L.mi_gpt_linear_decode.argtypes
        L.mi_gpt_linear_decode_q8.restype = C.c_int
        L.mi_gpt_linear_batch_q8.argtypes = [vp, vp] + L.mi_gpt_linear_batch.argtypes
        L.mi_gpt_linear_batch_q8.restype = C.c_int
    L.mi_gpt_bench_pick.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, C.POINTER(C.c_double)]
    L.mi_gpt_bench_pick.restype = C.c_int
    L.mi_bench_conv_gemm.argtypes = [C.c_int] * 9 + [C.POINTER(C.c_double)]
    L.mi_bench_conv_gemm.restype = C.c_int
    if hasattr(L, "mi_conv_gemm_plan"):
        L.mi_conv_gemm_plan.argtypes = [C.c_int] * 9 + [C.POINTER(C.c_int32), C.POINTER(C.c_int)]
        L.mi_conv_gemm_plan.restype = C.c_int
    L.mi_set_option.argtypes = [C.c_char_p, C.c_int64]; L.mi_set_option.restype = C.c_int
    L.mi_get_option.argtypes = [C.c_char_p, C.POINTER(C.c_int64)]; L.mi_get_option.restype = C.c_int
    L.mi_device_pci_bus_id.argtypes = [C.c_int, C.c_char_p, C.c_int]; L.mi_device_pci_bus_id.restype = C.c_int
    L.mi_prof_enable.argtypes = [C.c_int]; L.mi_prof_enable.restype = C.c_int
    L.mi_prof_reset.argtypes = []; L.mi_prof_reset.restype = C.c_int
    L.mi_prof_get.argtypes = [C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double),
                              C.POINTER(C.c_double)]
    L.mi_prof_get.restype = C.c_int
    L.mi_prof_kernel_count.argtypes = []; L.mi_prof_kernel_count.restype = C.c_int
    L.mi_prof_kernel_get.argtypes = [C.c_int, C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                     C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.mi_prof_kernel_get.restype = C.c_int
    _lib = L
    return L


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().mi_last_error().decode("utf-8", "replace")
        raise MiError(f"{what}: {msg} (code {rc})")


def f32p(a: np.ndarray):
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_float))


def i32p(a: np.ndarray):
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def init(device: int = 0) -> None:
    check(load().mi_init(device), "mi_init")


PROF_FAMILIES = ("conv_gemm", "aa_act", "conv_post", "attn", "norm", "other")


def prof_enable(families=()) -> None:
    """families: iterable of family names, or True for all, or False/() for off."""
    if families is True:
        mask = -1
    elif not families:
        mask = 0
    else:
        mask = 0
        for f in families:
            mask |= 1 << PROF_FAMILIES.index(f)
    load().mi_prof_enable(mask)


def prof_reset() -> None:
    check(load().mi_prof_reset(), "mi_prof_reset")


def prof_get(family: str) -> dict:
    ms, n, by, fl = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
    check(load().mi_prof_get(family.encode(), C.byref(ms), C.byref(n), C.byref(by), C.byref(fl)), "mi_prof_get")
    return {"ms": ms.value, "launches": n.value, "bytes": by.value, "flops": fl.value}


def prof_kernels() -> list:
    """Per-kernel-instantiation accumulators since the last prof_reset, sorted by total time (descending)."""
    L = load()
    out = []
    for i in range(L.mi_prof_kernel_count()):
        name, fam = C.create_string_buffer(256), C.create_string_buffer(32)
        ms, by, fl, n = C.c_double(0), C.c_double(0), C.c_double(0), C.c_int64(0)
        check(L.mi_prof_kernel_get(i, name, 256, fam, 32, C.byref(ms), C.byref(n), C.byref(by), C.byref(fl)), "mi_prof_kernel_get")
        out.append({"kernel": name.value.decode(), "family": fam.value.decode(), "ms": ms.value, "launches": int(n.value),
                    "bytes": by.value, "flops": fl.value})
    return sorted(out, key=lambda k: -k["ms"])


def bench_conv_gemm(dtype: str, B: int, T: int, Cin: int, N: int, taps: int = 1, dil: int = 1, with_res: bool = False,
                    iters: int = 20) -> float:
    """Average ms per launch of the implicit-GEMM kernel on random device data (tuning hook)."""
    ms = C.c_double()
    check(load().mi_bench_conv_gemm(DTYPES[dtype], B, T, Cin, N, taps, dil, int(with_res), iters, C.byref(ms)),
          "mi_bench_conv_gemm")
    return ms.value


GEMM_KINDS = ("none", "direct 256x32", "direct 128x64", "direct 128x128", "dma 64x64", "dma 64x64 fp16 pairs", "dma 128", "dma 128 ring4",
              "ph8", "x3p", "x3", "stream-k", "dma3 192", "dma3 256", "dma3 128")


def conv_gemm_plan(dtype: str, B: int, T: int, Cin: int, N: int, taps: int = 1, dil: int = 1, with_res: bool = False,
                   cus: int = 256) -> list:
    """Host only: what launch_conv_gemm would launch for bench_conv_gemm's arguments on a device of ``cus`` compute units, at the
    process's options.  One dict per launch (two when the rows are split): kind, Tm, Tn, RT, RC, lds_epi, use_buf, grid."""
    plans, n = (C.c_int32 * 20)(), C.c_int(0)
    check(load().mi_conv_gemm_plan(DTYPES.get(dtype, -1), B, T, Cin, N, taps, dil, int(with_res), cus, plans, C.byref(n)), "mi_conv_gemm_plan")
    keys = ("Tm", "Tn", "RT", "RC", "lds_epi", "use_buf")
    return [dict(zip(keys, plans[10 * i + 1:10 * i + 7]), kind=GEMM_KINDS[plans[10 * i]], grid=list(plans[10 * i + 7:10 * i + 10])) for i in range(n.value)]


def device_pci_bus_id(device: int) -> str:
    buf = C.create_string_buffer(64)
    check(load().mi_device_pci_bus_id(int(device), buf, 64), "mi_device_pci_bus_id")
    return buf.value.decode()


def set_option(key: str, value: int) -> None:
    check(load().mi_set_option(key.encode(), int(value)), "mi_set_option")


def get_option(key: str) -> int:
    """What the process runs with: the default, overridden by the environment (read once, at the first call into the library),
    overridden by set_option."""
    v = C.c_int64(0)
    check(load().mi_get_option(key.encode(), C.byref(v)), "mi_get_option")
    return int(v.value)
