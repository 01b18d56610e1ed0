"""GPU parity: the HIP F5-TTS path (through the C-ABI) against golden vectors from the reference's own
module/wrapper code and against the numpy oracle.

Tolerances (fp32 engine: exact-fp32 MFMA, fp32 softmax / norm statistics):
  tables / single ops      <= 1e-4 abs (summation order + libm vs torch transcendental differences)
  31-step sampler output   <= 2e-3 abs on O(2) values
  waveform                 <= 1e-3 RMS on the [-1,1] scale  (the north-star gate), asserted with headroom
bf16 / f16 engines: DiT operands rounded to 16 bit, fp32 residual stream -> waveform RMS gate 3e-2 (stated).
"""
import os

import numpy as np
import pytest

from mi355tts.config import F5Config
from mi355tts import weights as W
from mi355tts.f5 import F5Engine
from oracle import f5_np as O

pytestmark = pytest.mark.gpu


def rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))


def assert_logmel_close(got, ref, floor=2e-5, atol=2e-4, rtol=2e-4):
    """log(clamp(mel, 1e-5)): a difference of 1e-9 in a linear value next to the clamp floor is 1e-4 in its log, so the comparison
    is made where the reference sits above the floor (a blanket atol of 3e-3 hid everything else) — there the
    linear mel is a sum of >= 1 fp32 products and agrees to a few 1e-5 relative, i.e. a few 1e-5 absolute in the log."""
    m = ref > np.log(floor)
    assert m.mean() > 0.5, m.mean()
    np.testing.assert_allclose(np.asarray(got)[m], np.asarray(ref)[m], atol=atol, rtol=rtol)
    assert (np.asarray(got)[~m] < np.log(floor) + 0.7).all()       # below the floor on one side: at or near it on the other


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "f5_small.npz"))


@pytest.fixture(scope="module")
def small():
    cfg = F5Config.small()
    raw = W.synth_state(W.f5_spec(cfg), 9527)
    eng = F5Engine(cfg, raw, dtype="f32")
    yield cfg, W.fold_f5(cfg, raw), eng
    eng.close()


def test_param_count_and_tables(g, small):
    cfg, st, eng = small
    te, dt = eng.tables()
    np.testing.assert_allclose(dt, g["delta_t"], atol=2e-7)
    np.testing.assert_allclose(te, g["time_expand"], atol=5e-5)
    assert abs(float(dt.sum()) - 1.0) < 1e-6 and len(dt) == cfg.nfe_step - 1


def test_preprocess_golden(g, small):
    cfg, st, eng = small
    N = int(g["pre_N"])
    noise = g["dit_noise"]
    o = eng.preprocess(g["pre_audio"].reshape(1, 1, -1), g["pre_text_ids"].reshape(1, -1), np.array([N]), noise=noise)
    assert int(o["ref_signal_len"]) == int(g["pre_ref_signal_len"])
    assert o["rope_cos_q"].shape == (2, cfg.heads, N, 64) and o["rope_cos_k"].shape == (2, cfg.heads, 64, N)
    np.testing.assert_allclose(o["rope_cos_q"][1, 1], g["pre_rope_cos_q"], atol=1e-3)    # fp16-rounded tables (1 ulp_fp16)
    np.testing.assert_allclose(o["rope_sin_q"][0, 0], g["pre_rope_sin_q"], atol=1e-3)
    assert np.array_equal(o["noise"][0], noise)
    R = int(o["ref_signal_len"])
    assert_logmel_close(o["cat_mel_text"][0, :R, :100], g["pre_cat_mel_text"][:R, :100])
    assert np.all(o["cat_mel_text"][0, R:, :100] == 0.0)
    np.testing.assert_allclose(o["cat_mel_text"][0, :, 100:], g["pre_cat_mel_text"][:, 100:], atol=5e-5)
    np.testing.assert_allclose(o["cat_mel_text_drop"][0], g["pre_cat_mel_text_drop"], atol=5e-5)


def test_dit_eval_golden(g, small):
    cfg, st, eng = small
    pred = eng.dit_eval(g["dit_noise"][None], g["pre_cat_mel_text"][None], g["pre_cat_mel_text_drop"][None], 2)
    assert pred.shape == g["dit_pred_t2"].shape
    np.testing.assert_allclose(pred, g["dit_pred_t2"], atol=3e-4)


def test_step_and_loop_golden(g, small):
    cfg, st, eng = small
    x0, cmt, cmtd = g["dit_noise"][None], g["pre_cat_mel_text"][None], g["pre_cat_mel_text_drop"][None]
    x1, ts = eng.transformer_step(x0, cmt, cmtd, np.array([0], np.int32))
    assert int(ts[0]) == 1 and np.array_equal(x0[0], g["dit_noise"])          # inputs untouched
    np.testing.assert_allclose(x1[0], g["loop_step1"], atol=2e-4)
    # the reference loop: nfe_step - 1 calls, each feeding the previous output back
    x, t = x0, np.array([0], np.int32)
    for _ in range(cfg.nfe_step - 1):
        x, t = eng.transformer_step(x, cmt, cmtd, t)
    assert int(t[0]) == cfg.nfe_step - 1
    np.testing.assert_allclose(x[0], g["loop_final"], atol=2e-3)
    xs = eng.sample(x0, cmt, cmtd)                                               # device-resident loop == stepwise
    assert np.array_equal(xs, x)
    with pytest.raises(Exception):
        eng.transformer_step(x, cmt, cmtd, t)                                    # past the end of the grid


def test_batched_utterances_equal_single(g, small):
    cfg, st, eng = small
    x0, cmt, cmtd = g["dit_noise"][None], g["pre_cat_mel_text"][None], g["pre_cat_mel_text_drop"][None]
    x2 = np.concatenate([x0, x0[:, ::-1].copy()], 0)
    c2 = np.concatenate([cmt, cmt], 0)
    d2 = np.concatenate([cmtd, cmtd], 0)
    a = eng.sample(x2, c2, d2, n_steps=2)
    b0 = eng.sample(x0, cmt, cmtd, n_steps=2)
    b1 = eng.sample(x0[:, ::-1].copy(), cmt, cmtd, n_steps=2)
    assert np.array_equal(a[0], b0[0]) and np.array_equal(a[1], b1[0])


def test_f5_mel_handoff_to_bigvgan(g, small):
    """The "F5-TTS + BigVGAN" pipeline of the metric: mi_f5_synthesize_mel hands the generated frames on as (U, 100, N - R)
    channels-first fp32 = BigVGAN's mel_features.  It must be the sampler's own final state (== the reference sampler's
    fixture inside the loop tolerance), and a BigVGAN engine run on it must match the vocoder oracle run on the REFERENCE
    sampler's frames (fp32 engines: waveform <= 1e-3 RMS, the north-star gate)."""
    import dataclasses
    from mi355tts.config import BigVGANConfig
    from mi355tts.bigvgan import BigVGANVocoder
    from oracle import bigvgan_np as OB
    cfg, st, eng = small
    N, R = int(g["pre_N"]), int(g["pre_ref_signal_len"])
    audio, ids = g["pre_audio"].reshape(1, -1), g["pre_text_ids"].reshape(1, -1)
    noise = g["dit_noise"].reshape(1, N, cfg.mel_dim)
    mel = eng.synthesize_mel(audio, ids, N, noise=noise)
    assert mel.shape == (1, cfg.mel_dim, N - R) and mel.dtype == np.float32
    o = eng.preprocess(audio.reshape(1, 1, -1), ids, np.array([N]), noise=noise[0])
    xs = eng.sample(noise, o["cat_mel_text"], o["cat_mel_text_drop"])
    assert np.array_equal(mel[0], xs[0, R:].T)
    ref_mel = g["loop_final"][R:].T[None].astype(np.float32)
    np.testing.assert_allclose(mel, ref_mel, atol=5e-4)                             # the reference's own sampler state
    vcfg = dataclasses.replace(BigVGANConfig.small(), num_mels=cfg.mel_dim)
    vst = W.synth_state(W.bigvgan_spec(vcfg), 9527)
    voc = BigVGANVocoder(vcfg, vst, dtype="f32")
    wav = voc.run(mel)
    ref = OB.bigvgan_int16(vcfg, vst, ref_mel)
    assert wav.shape == ref.shape and rms(ref) > 100
    assert rms((wav.astype(np.float64) - ref.astype(np.float64)) / 32767.0) < 1e-3
    voc.close()


def test_decode_golden(g, small):
    cfg, st, eng = small
    R = int(g["pre_ref_signal_len"])
    w, wf = eng.decode(g["dec_in"][None], R, return_float=True)
    assert w.shape == (1, 1, g["dec_i16"].shape[0]) and w.dtype == np.int16
    assert rms(wf[0, 0] - g["dec_float"]) < 2e-5
    assert np.abs(w[0, 0].astype(np.int32) - g["dec_i16"].astype(np.int32)).max() <= 3


def test_end_to_end_golden_waveform(g, small):
    """audio + text in, waveform out, against the reference chain (noise injected)."""
    cfg, st, eng = small
    N = int(g["pre_N"])
    w = eng.synthesize(g["pre_audio"][None], g["pre_text_ids"][None], N, noise=g["dit_noise"][None])
    assert w.shape == (1, 1, g["e2e_i16"].shape[0])
    err = rms((w[0, 0].astype(np.float64) - g["e2e_i16"].astype(np.float64)) / 32767.0)
    assert err < 5e-4, err                                                      # north-star gate: 1e-3
    assert rms(g["e2e_i16"]) > 500


@pytest.mark.parametrize("dtype,gate", [("bf16", 3e-2), ("f16", 1e-2)])
def test_end_to_end_lowp(g, dtype, gate):
    cfg = F5Config.small()
    eng = F5Engine(cfg, W.synth_state(W.f5_spec(cfg), 9527), dtype=dtype)
    N = int(g["pre_N"])
    w = eng.synthesize(g["pre_audio"][None], g["pre_text_ids"][None], N, noise=g["dit_noise"][None])
    err = rms((w[0, 0].astype(np.float64) - g["e2e_i16"].astype(np.float64)) / 32767.0)
    assert err < gate, err
    eng.close()


def test_attention_against_oracle_ragged_lengths(small):
    """N not a multiple of the 64-key stage / 128-query tile; heads > 2 via a wider reduced model."""
    cfg = F5Config(dim=256, depth=1, heads=4, dim_head=64, text_dim=64, text_num_embeds=40, conv_layers=1,
                   pos_conv_groups=4, vocos_dim=64, vocos_intermediate=128, vocos_layers=1, nfe_step=4)
    raw = W.synth_state(W.f5_spec(cfg), 7)
    st = W.fold_f5(cfg, raw)
    eng = F5Engine(cfg, raw, dtype="f32")
    tables = O.time_tables(cfg, st)
    for N in (67, 130, 257):
        noise = W.synth_normal(3, f"n{N}", (N, cfg.mel_dim))
        cmt = W.synth_normal(4, f"c{N}", (N, cfg.mel_dim + cfg.text_dim), std=0.7)
        cmtd = W.synth_normal(5, f"d{N}", (N, cfg.mel_dim + cfg.text_dim), std=0.7)
        cos, sin = O.rope_tables(N, 64)
        ref = O.dit_forward(cfg, st, noise, cmt, cmtd, tables[2][1], cos, sin)
        pred = eng.dit_eval(noise[None], cmt[None], cmtd[None], 1)
        np.testing.assert_allclose(pred, ref, atol=3e-4)
    eng.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_attention_xcd_aware_workgroup_map_is_bit_neutral(dtype):
    """attn_xcd_map = 1 (the default: measured -1.3 % on the bf16 attention launch, -0.6 % in fp32) re-reads the workgroup
    ids so that the query tiles of a head share one XCD's L2.  Only WHICH workgroup computes a tile changes: the DiT evaluation
    must be bit-identical — 128-query and 64-query forms, key slices (N = 700 in fp32), batches of 1 and 2 utterances."""
    from mi355tts import _lib
    cfg = F5Config(dim=256, depth=1, heads=4, dim_head=64, text_dim=64, text_num_embeds=40, conv_layers=1,
                   pos_conv_groups=4, vocos_dim=64, vocos_intermediate=128, vocos_layers=1, nfe_step=4)
    eng = F5Engine(cfg, W.synth_state(W.f5_spec(cfg), 7), dtype=dtype)
    saved = {k: _lib.get_option(k) for k in ("attn_xcd_map",)}
    try:
        for U, N in ((1, 130), (2, 257), (1, 700)):
            noise = W.synth_normal(3, f"n{N}", (U, N, cfg.mel_dim))
            cmt = W.synth_normal(4, f"c{N}", (U, N, cfg.mel_dim + cfg.text_dim), std=0.7)
            cmtd = W.synth_normal(5, f"d{N}", (U, N, cfg.mel_dim + cfg.text_dim), std=0.7)
            _lib.set_option("attn_xcd_map", 0)
            ref = eng.dit_eval(noise, cmt, cmtd, 1)
            _lib.set_option("attn_xcd_map", 1)
            got = eng.dit_eval(noise, cmt, cmtd, 1)
            assert np.isfinite(ref).all() and np.array_equal(got, ref), (dtype, U, N)
    finally:
        for k, v in saved.items():
            _lib.set_option(k, v)
        eng.close()


def test_fp32_attention_split_products_match_native():
    """attn_f32_x3 = 1: q.k as exact three-way bf16 splits on the bf16 pipes; = 2: p.v as well (K / V^T split once per stage
    into bf16 planes in LDS, V transposed by the QKV epilogue); = 0: native fp32 MFMA.  All inside the DiT gate against the
    oracle and within 5e-5 of each other (N = 67 .. 700: 128-query and 64-query workgroups, key slices)."""
    from mi355tts import _lib
    cfg = F5Config(dim=256, depth=1, heads=4, dim_head=64, text_dim=64, text_num_embeds=40, conv_layers=1,
                   pos_conv_groups=4, vocos_dim=64, vocos_intermediate=128, vocos_layers=1, nfe_step=4)
    raw = W.synth_state(W.f5_spec(cfg), 7)
    st = W.fold_f5(cfg, raw)
    eng = F5Engine(cfg, raw, dtype="f32")
    tables = O.time_tables(cfg, st)
    saved = {k: _lib.get_option(k) for k in ("attn_f32_x3", "attn_split")}
    try:
        for N in (67, 257, 700):
            noise = W.synth_normal(3, f"n{N}", (N, cfg.mel_dim))
            cmt = W.synth_normal(4, f"c{N}", (N, cfg.mel_dim + cfg.text_dim), std=0.7)
            cmtd = W.synth_normal(5, f"d{N}", (N, cfg.mel_dim + cfg.text_dim), std=0.7)
            cos, sin = O.rope_tables(N, 64)
            ref = O.dit_forward(cfg, st, noise, cmt, cmtd, tables[2][1], cos, sin)
            got = {}
            for split in (1, 2, 0):                            # 64-query key-split workgroups / 128-query + key slices / the 128-query form of large batches
                _lib.set_option("attn_split", split)
                for x3 in (2, 1, 0):
                    _lib.set_option("attn_f32_x3", x3)
                    got[x3] = eng.dit_eval(noise[None], cmt[None], cmtd[None], 1)
                    np.testing.assert_allclose(got[x3], ref, atol=3e-4)
                    assert np.array_equal(got[x3], eng.dit_eval(noise[None], cmt[None], cmtd[None], 1))
                assert np.abs(got[1] - got[0]).max() < 5e-5 and np.abs(got[2] - got[0]).max() < 5e-5
    finally:
        for k, v in saved.items():
            _lib.set_option(k, v)
        eng.close()


def test_attention_uneven_key_slices_longest_first():
    """Round 6: the fp32 128-query attention launch cuts the 64-key stages into UNEVEN slices, longest first (attn_pick_slices: the
    z-major dispatch order is then list scheduling on the 3 x CUs workgroup slots; N = 1126: 7 + 7 + 2 + 2 stages instead of 6 + 6 + 6).
    Same merge as the even slices: against the oracle, against the even slices (attn_lpt = 0) and identical run to run, at lengths whose
    stage counts split differently."""
    from mi355tts import _lib
    cfg = F5Config(dim=256, depth=1, heads=4, dim_head=64, text_dim=64, text_num_embeds=40, conv_layers=1,
                   pos_conv_groups=4, vocos_dim=64, vocos_intermediate=128, vocos_layers=1, nfe_step=4)
    raw = W.synth_state(W.f5_spec(cfg), 7)
    st = W.fold_f5(cfg, raw)
    eng = F5Engine(cfg, raw, dtype="f32")
    tables = O.time_tables(cfg, st)
    saved = {k: _lib.get_option(k) for k in ("attn_lpt",)}
    try:
        for N in (257, 700, 1126):
            noise = W.synth_normal(3, f"n{N}", (N, cfg.mel_dim))
            cmt = W.synth_normal(4, f"c{N}", (N, cfg.mel_dim + cfg.text_dim), std=0.7)
            cmtd = W.synth_normal(5, f"d{N}", (N, cfg.mel_dim + cfg.text_dim), std=0.7)
            cos, sin = O.rope_tables(N, 64)
            ref = O.dit_forward(cfg, st, noise, cmt, cmtd, tables[2][1], cos, sin)
            _lib.set_option("attn_lpt", 0)
            even = eng.dit_eval(noise[None], cmt[None], cmtd[None], 1)
            _lib.set_option("attn_lpt", 1)
            a = eng.dit_eval(noise[None], cmt[None], cmtd[None], 1)
            for _ in range(3):
                assert np.array_equal(a, eng.dit_eval(noise[None], cmt[None], cmtd[None], 1)), N
            np.testing.assert_allclose(a, ref, atol=3e-4)
            assert np.abs(a - even).max() < 1e-4, N
    finally:
        for k, v in saved.items():
            _lib.set_option(k, v)
        eng.close()


@pytest.mark.parametrize("dtype,tol,split", [("f32", 3e-4, 1), ("f32", 3e-4, 2), ("f16", 1.5e-2, 1)])
def test_attention_key_slices_agree(dtype, tol, split):
    """Key-sliced attention (gridDim.z slices of the 64-key stages, last-arriver merge in slice order): every slice count,
    including slices that get no stage at all, gives the unsliced result within rounding and is identical run to run.
    split = 1: 64-query workgroups whose wave pairs share the keys; 2 (fp32 pairs kernel): 128-query workgroups, four
    32-query groups per slice."""
    from mi355tts import _lib
    saved = {k: _lib.get_option(k) for k in ("attn_z_force", "attn_split")}
    _lib.set_option("attn_split", split)
    cfg = F5Config(dim=256, depth=1, heads=4, dim_head=64, text_dim=64, text_num_embeds=40, conv_layers=1,
                   pos_conv_groups=4, vocos_dim=64, vocos_intermediate=128, vocos_layers=1, nfe_step=4)
    raw = W.synth_state(W.f5_spec(cfg), 7)
    st = W.fold_f5(cfg, raw)
    eng = F5Engine(cfg, raw, dtype=dtype)
    tables = O.time_tables(cfg, st)
    try:
        for N in (130, 257, 700):                              # 3 / 5 / 11 stages of 64 keys: N = 130 leaves the fourth slice empty
            noise = W.synth_normal(3, f"n{N}", (N, cfg.mel_dim))
            cmt = W.synth_normal(4, f"c{N}", (N, cfg.mel_dim + cfg.text_dim), std=0.7)
            cmtd = W.synth_normal(5, f"d{N}", (N, cfg.mel_dim + cfg.text_dim), std=0.7)
            cos, sin = O.rope_tables(N, 64)
            ref = O.dit_forward(cfg, st, noise, cmt, cmtd, tables[2][1], cos, sin)
            outs = []
            for z in (1, 2, 3, 4):
                _lib.set_option("attn_z_force", z)
                a = eng.dit_eval(noise[None], cmt[None], cmtd[None], 1)
                for _ in range(3):
                    assert np.array_equal(a, eng.dit_eval(noise[None], cmt[None], cmtd[None], 1)), (N, z)
                if dtype == "f32":
                    np.testing.assert_allclose(a, ref, atol=tol)
                else:
                    assert rms(a - ref) / rms(ref) < tol
                outs.append(a)
            for a in outs[1:]:
                assert np.abs(a - outs[0]).max() < (1e-4 if dtype == "f32" else 0.1)
    finally:
        for k, v in saved.items():
            _lib.set_option(k, v)
        eng.close()


@pytest.mark.parametrize("dtype,tol", [("f16", 1.5e-2), ("bf16", 8e-2)])
def test_dit_16bit_ragged_batch_against_oracle(dtype, tol):
    """16-bit DiT evaluation, two utterances flattened into the GEMM M axis with an odd token count: the LDS-staged QKV
    epilogue (RoPE on 8-column chunks, V written transposed with lane = key) sees item boundaries inside its 64-row
    tiles and key offsets that are not multiples of 8."""
    cfg = F5Config(dim=256, depth=2, heads=4, dim_head=64, text_dim=64, text_num_embeds=40, conv_layers=1,
                   pos_conv_groups=4, vocos_dim=64, vocos_intermediate=128, vocos_layers=1, nfe_step=4)
    raw = W.synth_state(W.f5_spec(cfg), 7)
    st = W.fold_f5(cfg, raw)
    eng = F5Engine(cfg, raw, dtype=dtype)
    tables = O.time_tables(cfg, st)
    for N in (67, 131, 257):
        noise = np.stack([W.synth_normal(3 + u, f"n{N}", (N, cfg.mel_dim)) for u in range(2)])
        cmt = np.stack([W.synth_normal(14 + u, f"c{N}", (N, cfg.mel_dim + cfg.text_dim), std=0.7) for u in range(2)])
        cmtd = np.stack([W.synth_normal(25 + u, f"d{N}", (N, cfg.mel_dim + cfg.text_dim), std=0.7) for u in range(2)])
        cos, sin = O.rope_tables(N, 64)
        pred = eng.dit_eval(noise, cmt, cmtd, 1)
        for u in range(2):
            ref = O.dit_forward(cfg, st, noise[u], cmt[u], cmtd[u], tables[2][1], cos, sin)
            got = pred[2 * u:2 * u + 2]
            assert got.shape == ref.shape
            assert rms(got - ref) / rms(ref) < tol, (N, u, rms(got - ref) / rms(ref))
            assert np.abs(got - ref).max() < 12 * tol * rms(ref), (N, u)
    eng.close()


def test_bad_arguments(small):
    cfg, st, eng = small
    with pytest.raises(ValueError):
        eng.decode(np.zeros((1, 10, cfg.mel_dim + 1), np.float32), 3)
    from mi355tts._lib import MiError
    with pytest.raises(MiError):                       # max_duration shorter than the reference audio
        eng.preprocess(np.zeros(8192, np.int16), np.zeros(4, np.int32), 8)
    with pytest.raises(MiError):                       # text id outside the embedding table
        eng.preprocess(np.zeros(8192, np.int16), np.full(4, 10 ** 6, np.int32), 60)


# ---------------------------------------------------------------------------------------------
# BASELINE.json size (F5Config(): 22 DiT blocks, N = 1126 frames from 6 s of reference audio): the numpy oracle needs
# ~8 minutes for the 31 evaluations, so the full size is held by size-independent properties instead:
#   * utterances are independent: a batch of two different utterances == the two run alone,
#     which exercises the batch-flattened GEMMs, the per-(item, head) attention grid and the ragged 1126 = 8 x 128 + 102
#     tile tails at the real shape;
#   * the same call twice is bit-identical (first call eager, later calls replay the captured hipGraph);
#   * the bf16 engine (16-bit LDS-DMA GEMMs, fast GELU, packed RoPE table, 16-bit attention) stays inside the stated
#     low-precision gate of the fp32 engine's waveform.
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full():
    cfg = F5Config()
    raw = W.synth_state(W.f5_spec(cfg), 9527)
    audio, ids, N, noise = W.f5_synthetic_inputs(cfg, 8, 0)
    return cfg, raw, audio, ids, N, noise


def test_full_size_batch_invariance_determinism_and_lowp_gate(full):
    cfg, raw, audio, ids, N, noise = full
    audio, ids, noise = audio[:2], ids[:2], noise[:2]
    assert N == 1126 and audio.shape == (2, 144000)
    e32 = F5Engine(cfg, raw, dtype="f32")
    w_pair = e32.synthesize(audio, ids, N, noise=noise)
    assert w_pair.shape == (2, 1, (N - 563 - 1) * cfg.hop_length) and w_pair.dtype == np.int16
    w0 = e32.synthesize(audio[:1], ids[:1], N, noise=noise[:1])
    w1 = e32.synthesize(audio[1:], ids[1:], N, noise=noise[1:])
    # fp32, same kernels and tile shapes per row: identical up to the int16 truncation boundary
    for wp, ws in ((w_pair[0], w0[0]), (w_pair[1], w1[0])):
        d = np.abs(wp.astype(np.int32) - ws.astype(np.int32))
        assert d.max() <= 2 and (d > 0).mean() < 0.01
    assert rms(w0) > 300 and not np.array_equal(w0, w1)                  # neither silent nor saturated, and really different
    assert np.abs(w0.astype(np.int32)).max() < 32767
    w0b = e32.synthesize(audio[:1], ids[:1], N, noise=noise[:1])          # replayed hipGraph
    w0c = e32.synthesize(audio[:1], ids[:1], N, noise=noise[:1])
    assert np.array_equal(w0b, w0c)
    d = np.abs(w0.astype(np.int32) - w0b.astype(np.int32))
    assert d.max() <= 2
    e32.close()
    e16 = F5Engine(cfg, raw, dtype="bf16")
    wb = e16.synthesize(audio[:1], ids[:1], N, noise=noise[:1])
    err = rms((wb.astype(np.float64) - w0.astype(np.float64)) / 32767.0)
    assert err < 1.5e-3, err            # achieved 2.5e-4 (profiles/r3); the stated low-precision gate used to be 3e-2
    e16.close()


# ---------------------------------------------------------------------------------------------
# BASELINE.json size against the REFERENCE itself: tests/golden/f5_full.npz holds the outputs of the reference chain
# (F5Preprocess -> 31 x F5Transformer -> F5Decode, Export_F5.py:98-203 over modeling_modified/F5 + vocos + STFT_Process)
# at F5Config() / N = 1126 on utterance 0 of the bench inputs (tests/golden/make_golden_full.py, ~2 min of torch-CPU).
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gfull(golden_dir):
    return np.load(os.path.join(golden_dir, "f5_full.npz"))


@pytest.mark.parametrize("form", ["fp16-pairs", "fp16-pairs, row-norm launches", "bf16x3-splits", "native-fp32-mfma"])
def test_full_size_fp32_against_reference_fixture(full, gfull, form):
    """configs[2]: fp32, one utterance, NFE grid 32 — the north-star gate (waveform <= 1e-3 RMS) on the north-star config.
    Every fp32 form of the engine, selected per ENGINE (F5Config.f32_arithmetic / adaln_fold, round 4): the default (linear
    layers, attention and position convolution as fp16 {hi, lo} pairs, AdaLN folded into the GEMM epilogues), the same with
    row-norm launches instead of the fold, the linear layers as three bf16 planes (round 3's first form) and the native fp32
    MFMA (what bench.py times as secondary.f5_f32_native_mfma)."""
    import dataclasses
    cfg = full[0]
    kind = {"fp16-pairs": "fp16x2-pairs", "fp16-pairs, row-norm launches": "fp16x2-pairs", "bf16x3-splits": "bf16x3",
            "native-fp32-mfma": "native-fp32-mfma"}[form]
    cfg2 = dataclasses.replace(cfg, f32_arithmetic=kind, adaln_fold=False if "row-norm" in form else None)
    _full_size_fp32_body((cfg2,) + tuple(full[1:]), gfull, form)


def _full_size_fp32_body(full, gfull, form):
    cfg, raw, audio, ids, N, noise = full
    assert int(gfull["N"]) == N
    eng = F5Engine(cfg, raw, dtype="f32")
    o = eng.preprocess(audio[0].reshape(1, 1, -1), ids[0].reshape(1, -1), np.array([N]), noise=noise[0])
    R = int(o["ref_signal_len"])
    assert R == int(gfull["ref_signal_len"]) == 563
    assert_logmel_close(o["cat_mel_text"][0, :R, :100], gfull["pre_cat_mel_text"][:R, :100])
    np.testing.assert_allclose(o["cat_mel_text"][0, :, 100:], gfull["pre_cat_mel_text"][:, 100:], atol=1e-4)
    pred = eng.dit_eval(noise[:1], o["cat_mel_text"], o["cat_mel_text_drop"], 7)
    e_pred = rms(pred - gfull["dit_pred_t7"]) / rms(gfull["dit_pred_t7"])
    assert pred.shape == (2, N, cfg.mel_dim) and e_pred < 1e-4, e_pred
    assert np.abs(pred - gfull["dit_pred_t7"]).max() < 2e-3
    x1, ts = eng.transformer_step(noise[:1], o["cat_mel_text"], o["cat_mel_text_drop"], np.array([0], np.int32))
    np.testing.assert_allclose(x1[0], gfull["loop_step1"], atol=5e-4)
    xs = eng.sample(noise[:1], o["cat_mel_text"], o["cat_mel_text_drop"])
    e_loop = rms(xs[0] - gfull["loop_final"]) / rms(gfull["loop_final"])
    assert e_loop < 1e-3, e_loop
    w = eng.synthesize(audio[:1], ids[:1], N, noise=noise[:1])
    assert w.shape == (1, 1, gfull["e2e_i16"].shape[0])
    err = rms((w[0, 0].astype(np.float64) - gfull["e2e_i16"].astype(np.float64)) / 32767.0)
    assert err < 1e-3, err                                               # THE north-star gate
    assert rms(gfull["e2e_i16"]) > 500
    assert eng.info()["f32_arithmetic"] == cfg.f32_arithmetic and eng.info()["saturation_events"] == 0
    eng.close()
    print(f"F5 full size fp32 ({form}) vs reference: DiT eval rel {e_pred:.2e}, "
          f"31-step state rel {e_loop:.2e}, waveform rms {err:.2e}")


def test_full_size_fp32_fused_producers_are_bit_neutral(full):
    """Round 3 moved the split of the fp32 operands out of the consumers into their producers (rownorm / attention / FF1
    epilogue write the next GEMM's panel planes, the QKV epilogue writes K and V^T as planes for attention).  The split is a
    function of the fp32 value alone, so WHERE it happens must not change a bit: with the three-bf16-plane attention format
    (attn_f32_planes = 3, the only one the in-kernel split produces) K / V planes on vs off give identical DiT evaluations
    (one and three utterances: both attention tilings).  The default fp16-pair format (attn_f32_planes = 2) is other
    arithmetic: it must sit as close to the three-plane result as the native fp32 MFMA path does."""
    from mi355tts import _lib
    cfg, raw, audio, ids, N, noise = full
    eng = F5Engine(cfg, raw, dtype="f32")
    saved = {k: _lib.get_option(k) for k in ("attn_kv_planes", "attn_f32_planes")}
    try:
        for U in (1, 3):
            o = [eng.preprocess(audio[u].reshape(1, 1, -1), ids[u].reshape(1, -1), np.array([N]), noise=noise[u]) for u in range(U)]
            cmt = np.concatenate([x["cat_mel_text"] for x in o]); cmtd = np.concatenate([x["cat_mel_text_drop"] for x in o])
            pairs = eng.dit_eval(noise[:U], cmt, cmtd, 5)
            _lib.set_option("attn_f32_planes", 3)
            a = eng.dit_eval(noise[:U], cmt, cmtd, 5)
            _lib.set_option("attn_kv_planes", 0)
            b = eng.dit_eval(noise[:U], cmt, cmtd, 5)
            _lib.set_option("attn_kv_planes", 1)
            _lib.set_option("attn_f32_planes", 2)
            assert np.array_equal(a, b), (U, np.abs(a - b).max())
            e = rms(pairs - a) / rms(a)
            print(f"U={U}: DiT evaluation, fp16-pair attention against three-plane attention: rel rms {e:.2e}")
            assert e < 2e-6 and not np.array_equal(pairs, a), e
    finally:
        for k, v in saved.items():
            _lib.set_option(k, v)
        eng.close()


# 1037 / 1152: the shortest and the longest utterance whose 2 N rows the exact-fit tiling takes in one round (>= 90 % of 16 x 144 rows);
# 1153: one frame more, 17 row groups = 53 % of two rounds, back on the stream-K kernel
# 1268: the reference's own zh.wav prompt length, on stream-K
@pytest.mark.parametrize("N", [701, 1015, 1037, 1152, 1153, 1268, 1280])
def test_full_size_fp32_other_lengths_default_forms_against_native(full, N):
    """The full-width DiT at frame counts other than the bench's 1126 — odd ones (K / V^T plane rows, the second batch item's
    rows and the last 128-row panel all start at odd offsets), one that fills whole panels — default arithmetic (fp16-pair
    linear layers, pre-split K / V^T, fp16-pair attention, pair-split position convolution) against the native fp32 MFMA
    forms of the same engine, one evaluation and two utterances; and both utterances against the fp32 oracle (the two engine
    forms share the input embedding, position convolution, time MLP, AdaLN-final and proj_out, where a bug would cancel)."""
    from mi355tts import _lib
    cfg, raw, audio, ids, _, _ = full
    noise = np.stack([W.synth_normal(77 + u, "noise_n", (N, cfg.mel_dim)) for u in range(2)])
    eng = F5Engine(cfg, raw, dtype="f32")
    saved = {k: _lib.get_option(k) for k in ("gemm_f32_x3", "attn_f32_x3", "gemm_f32_n64_pairs")}
    try:
        o = [eng.preprocess(audio[u].reshape(1, 1, -1), ids[u].reshape(1, -1), np.array([N]), noise=noise[u]) for u in range(2)]
        cmt = np.concatenate([x["cat_mel_text"] for x in o]); cmtd = np.concatenate([x["cat_mel_text_drop"] for x in o])
        a = eng.dit_eval(noise, cmt, cmtd, 3)
        a1 = eng.dit_eval(noise[:1], cmt[:1], cmtd[:1], 3)
        _lib.set_option("gemm_f32_x3", 0); _lib.set_option("attn_f32_x3", 0); _lib.set_option("gemm_f32_n64_pairs", 0)
        b = eng.dit_eval(noise, cmt, cmtd, 3)
    finally:
        for k, v in saved.items():
            _lib.set_option(k, v)
        eng.close()
    assert a.shape == (4, N, cfg.mel_dim) and np.isfinite(a).all()
    e = rms(a - b) / rms(b)
    print(f"N = {N}: default forms against native fp32 MFMA, DiT evaluation: rel rms {e:.2e}")
    assert e < 3e-6, e
    assert rms(a[:2] - a1) / rms(a1) < 3e-6                    # one utterance alone: other tile counts, same values
    st = W.fold_f5(cfg, raw)
    t_emb = O.time_tables(cfg, st)[2][3]
    cos, sin = O.rope_tables(N, cfg.dim_head)
    for u in range(2):
        ref = O.dit_forward(cfg, st, noise[u], cmt[u], cmtd[u], t_emb, cos, sin)
        e_o = rms(a[2 * u:2 * u + 2] - ref) / rms(ref)
        print(f"N = {N}: utterance {u}, default forms against the oracle: rel rms {e_o:.2e}")
        assert e_o < 3.5e-6, (u, e_o)                           # achieved 1.09e-6 .. 1.13e-6 at every N


@pytest.mark.parametrize("N", [1126, 333])
def test_fp32_position_convolution_weights_split_at_load(full, N):
    """ConvPositionEmbedding (modules.py:167-190: two grouped k = 31 convolutions + Mish) on fp16 pairs: the round-6 kernel takes its
    weights pre-split at load and keeps two taps in flight per workgroup (gconv_pairs2_kernel); the round-3 kernel re-splits them
    per launch (option gconv_two_taps = 0).  Same operands, same products, another summation order (even taps + odd taps): the
    evaluations agree to fp32 round-off, at the bench length and at one whose last row tile is cut (333 = 192 + 141)."""
    from mi355tts import _lib
    cfg, raw, audio, ids, _, _ = full
    noise = np.stack([W.synth_normal(31 + u, "noise_gc", (N, cfg.mel_dim)) for u in range(2)])
    eng = F5Engine(cfg, raw, dtype="f32")
    outs, kernels = {}, {}
    saved = {k: _lib.get_option(k) for k in ("gconv_two_taps",)}
    try:
        o = [eng.preprocess(audio[u].reshape(1, 1, -1)[..., :24000 * 2], ids[u].reshape(1, -1)[:, :40], np.array([N]), noise=noise[u]) for u in range(2)]
        cmt = np.concatenate([x["cat_mel_text"] for x in o]); cmtd = np.concatenate([x["cat_mel_text_drop"] for x in o])
        for on in (1, 0):
            _lib.set_option("gconv_two_taps", on)
            _lib.prof_reset(); _lib.prof_enable(["conv_gemm"])
            try:
                outs[on] = eng.dit_eval(noise, cmt, cmtd, 9)
            finally:
                _lib.prof_enable(())
            kernels[on] = [k["kernel"] for k in _lib.prof_kernels()]
        assert eng.info()["saturation_events"] == 0
    finally:
        for k, v in saved.items():
            _lib.set_option(k, v)
        eng.close()
    assert any("gconv_pairs2_kernel" in k for k in kernels[1]) and not any("gconv_pairs2_kernel" in k for k in kernels[0]), kernels
    assert any("gconv_pairs_kernel" in k for k in kernels[0]), kernels[0]
    e = rms(outs[1] - outs[0]) / rms(outs[0])
    print(f"N = {N}: position convolution, weights split at load against per launch: rel rms {e:.2e}")
    assert np.isfinite(outs[1]).all() and e < 2e-6, e


@pytest.mark.parametrize("x3d", [0, 1])
def test_two_fp32_handles_on_two_threads_stream_k_and_exact_fit(full, x3d):
    """the stream-K fix-up of linear_x3p_kernel (x3d = 0: owners spin, bounded, on their contributors' flags) rests
    on the workgroups of ONE launch being dispatched in order — with two handles on two streams two such grids share the chip.
    Two full-width fp32 engines, each driven by its own thread through three evaluations and three Euler steps at once: no watchdog
    trip (f5_run_checked raises on one), no dead-lock, and every result equal, bit for bit, to what the same handle computes alone.
    x3d = 1: the same with the exact-fit kernels, which have no cross-workgroup hand-off at all."""
    import threading
    from mi355tts import _lib
    cfg, raw, audio, ids, _, _ = full
    N = 1126
    engs = [F5Engine(cfg, raw, dtype="f32") for _ in range(2)]
    saved = {k: _lib.get_option(k) for k in ("gemm_x3d",)}
    _lib.set_option("gemm_x3d", x3d)
    try:
        inputs = []
        for u, eng in enumerate(engs):
            noise = W.synth_normal(61 + u, "noise_2h", (1, N, cfg.mel_dim))
            o = eng.preprocess(audio[u].reshape(1, 1, -1), ids[u].reshape(1, -1), np.array([N]), noise=noise[0])
            inputs.append((noise, o["cat_mel_text"], o["cat_mel_text_drop"]))

        def run(eng, inp):
            noise, cmt, cmtd = inp
            outs = [eng.dit_eval(noise, cmt, cmtd, k) for k in (0, 7, 30)]
            x = noise.copy()
            for k in range(3):
                x, _ = eng.transformer_step(x, cmt, cmtd, k)
            return outs + [np.asarray(x)]
        want = [run(e, i) for e, i in zip(engs, inputs)]           # each handle alone
        got, errs = [None, None], []

        def work(j):
            try:
                for _ in range(2):
                    got[j] = run(engs[j], inputs[j])
            except Exception as e:                      # pragma: no cover
                errs.append(e)
        th = [threading.Thread(target=work, args=(j,)) for j in range(2)]
        [t.start() for t in th]
        [t.join(600) for t in th]
        assert not any(t.is_alive() for t in th), "dead-lock"
        assert not errs, errs
        for j in range(2):
            for a, b in zip(got[j], want[j]):
                assert np.array_equal(a, b)
            assert engs[j].info()["saturation_events"] == 0
    finally:
        for k, v in saved.items():
            _lib.set_option(k, v)
        for e in engs: e.close()


def test_fp32_output_projection_in_k_slices(full, monkeypatch):
    """proj_out (dit.py: Linear(dim, mel) behind AdaLN-final) runs on fp32 engines as four K slices — a grouped launch whose partial
    sums lie side by side and are added in slice order by the consumers (cfg_update_kernel inside the loop, F5::pred_rows for
    mi_f5_dit_eval).  Against an engine built with MI355TTS_PROJ_PARTS=1 (one slice): the evaluation and four Euler steps of the loop
    agree to fp32 round-off."""
    cfg, raw, audio, ids, _, _ = full
    N = 600
    noise = np.stack([W.synth_normal(41 + u, "noise_pp", (N, cfg.mel_dim)) for u in range(2)])
    outs = {}
    for parts in ("4", "1"):
        monkeypatch.setenv("MI355TTS_PROJ_PARTS", parts)
        eng = F5Engine(cfg, raw, dtype="f32")
        try:
            o = [eng.preprocess(audio[u].reshape(1, 1, -1)[..., :72000], ids[u].reshape(1, -1), np.array([N]), noise=noise[u]) for u in range(2)]
            cmt = np.concatenate([x["cat_mel_text"] for x in o]); cmtd = np.concatenate([x["cat_mel_text_drop"] for x in o])
            pred = eng.dit_eval(noise, cmt, cmtd, 2)
            x = noise.copy()
            for k in range(4):
                x, _ = eng.transformer_step(x, cmt, cmtd, k)
            outs[parts] = (pred, np.asarray(x))
        finally:
            eng.close()
    for a, b in zip(outs["4"], outs["1"]):
        assert a.shape == b.shape and np.isfinite(a).all()
        e = rms(a - b) / rms(b)
        print(f"proj_out in four K slices against one: rel rms {e:.2e}")
        assert e < 2e-6, e


@pytest.mark.parametrize("dtype,tol", [("bf16", 6e-3), ("f16", 8e-4)])
def test_16bit_position_convolution_from_weight_images(full, dtype, tol):
    """ConvPositionEmbedding on the 16-bit engines (csrc/gconv16.hip: weight images built at load, input rows staged once, two taps in
    flight) against the generic tile kernel it replaces (option gconv16 = 0): the same 16-bit operands and fp32 accumulation in another
    order, so the DiT evaluation differs by the roundings of the 16-bit intermediates only; two utterances, a cut last row tile."""
    from mi355tts import _lib
    cfg, raw, audio, ids, _, _ = full
    N = 700
    noise = np.stack([W.synth_normal(71 + u, "noise_g16", (N, cfg.mel_dim)) for u in range(2)])
    eng = F5Engine(cfg, raw, dtype=dtype)
    outs, kernels = {}, {}
    saved = {k: _lib.get_option(k) for k in ("gconv16",)}
    try:
        o = [eng.preprocess(audio[u].reshape(1, 1, -1)[..., :96000], ids[u].reshape(1, -1), np.array([N]), noise=noise[u]) for u in range(2)]
        cmt = np.concatenate([x["cat_mel_text"] for x in o]); cmtd = np.concatenate([x["cat_mel_text_drop"] for x in o])
        for on in (1, 0):
            _lib.set_option("gconv16", on)
            _lib.prof_reset(); _lib.prof_enable(["conv_gemm"])
            try:
                outs[on] = eng.dit_eval(noise, cmt, cmtd, 4)
            finally:
                _lib.prof_enable(())
            kernels[on] = [k["kernel"] for k in _lib.prof_kernels()]
    finally:
        for k, v in saved.items():
            _lib.set_option(k, v)
        eng.close()
    assert any("gconv16_kernel" in k for k in kernels[1]) and not any("gconv16_kernel" in k for k in kernels[0]), kernels
    e = rms(outs[1] - outs[0]) / rms(outs[0])
    print(f"{dtype}: position convolution from weight images against the tile kernel: rel rms {e:.2e}")
    assert np.isfinite(outs[1]).all() and e < tol, e


def test_fp32_input_projection_padded_to_whole_chunks(full, monkeypatch):
    """fp32 engines pad K of the input projection (2 * mel + text_dim = 712, dit.py InputEmbedding.proj) to 768 with zero
    weight columns and a zeroed tail of the cat buffer's rows, so that the layer runs on the panel-plane kernel (csrc/f5.hip,
    F5::cat_ld).  Against the unpadded engine (MI355TTS_CAT_PAD=0 at construction: the native fp32 small-tile kernel): the same
    evaluation to fp32 round-off, for one and for two utterances, and the padded engine's profile shows the layer on
    linear_x3d_kernel<64, rows out> (two launches per evaluation: this one and the last block's FF2)."""
    from mi355tts import _lib
    cfg, raw, audio, ids, _, _ = full
    N = 1126
    noise = np.stack([W.synth_normal(5 + u, "noise_pad", (N, cfg.mel_dim)) for u in range(2)])
    outs, kernels = {}, {}
    for pad in ("1", "0"):
        monkeypatch.setenv("MI355TTS_CAT_PAD", pad)
        eng = F5Engine(cfg, raw, dtype="f32")
        try:
            o = [eng.preprocess(audio[u].reshape(1, 1, -1), ids[u].reshape(1, -1), np.array([N]), noise=noise[u]) for u in range(2)]
            cmt = np.concatenate([x["cat_mel_text"] for x in o]); cmtd = np.concatenate([x["cat_mel_text_drop"] for x in o])
            one = eng.dit_eval(noise[:1], cmt[:1], cmtd[:1], 5)
            _lib.prof_reset(); _lib.prof_enable(["conv_gemm"])
            try:
                again = eng.dit_eval(noise[:1], cmt[:1], cmtd[:1], 5)
            finally:
                _lib.prof_enable(())
            kernels[pad] = {k["kernel"]: k["launches"] for k in _lib.prof_kernels()}
            assert np.array_equal(one, again)
            outs[pad] = (one, eng.dit_eval(noise, cmt, cmtd, 5))
            assert eng.info()["saturation_events"] == 0
        finally:
            eng.close()
    for a, b in zip(outs["1"], outs["0"]):
        assert a.shape == b.shape and np.isfinite(a).all()
        e = rms(a - b) / rms(b)
        print(f"padded against unpadded input projection: rel rms {e:.2e}")
        assert e < 3e-6, e
    rows_out = [n for k, n in kernels["1"].items() if "linear_x3d_kernel<64, rows out>" in k]
    assert rows_out == [2], kernels["1"]
    assert [n for k, n in kernels["0"].items() if "linear_x3d_kernel<64, rows out>" in k] == [1], kernels["0"]


@pytest.mark.parametrize("dtype,gate", [("bf16", 1.5e-3), ("f16", 3e-4)])        # achieved (profiles/r3): 2.5e-4 / 3.4e-5
def test_full_size_lowp_u8_against_reference_fixture(full, gfull, dtype, gate):
    """configs[3] shard: 8 utterances per GPU in one batch, 16-bit DiT operands.  Utterance 0 is the reference fixture's
    utterance: waveform inside the stated low-precision gate of the REFERENCE waveform; every utterance equals its own
    single-utterance run inside the same gate (different tile / split-K configurations at M = 18016 rows vs 2252)."""
    cfg, raw, audio, ids, N, noise = full
    eng = F5Engine(cfg, raw, dtype=dtype)
    w8 = eng.synthesize(audio, ids, N, noise=noise)
    assert w8.shape == (8, 1, gfull["e2e_i16"].shape[0])
    err = rms((w8[0, 0].astype(np.float64) - gfull["e2e_i16"].astype(np.float64)) / 32767.0)
    assert err < gate, err
    w1 = eng.synthesize(audio[5:6], ids[5:6], N, noise=noise[5:6])
    e5 = rms((w8[5, 0].astype(np.float64) - w1[0, 0].astype(np.float64)) / 32767.0)
    assert e5 < gate, e5
    for u in range(8):
        assert rms(w8[u]) > 300
        assert u == 0 or not np.array_equal(w8[u], w8[0])
    eng.close()
    print(f"F5 full size {dtype} U=8 vs reference: waveform rms {err:.2e} (gate {gate}), item 5 batch vs alone {e5:.2e}")


@pytest.fixture(scope="module")
def gfull16(golden_dir):
    return np.load(os.path.join(golden_dir, "f5_full_fp16.npz"))


def test_full_size_reference_fp16_transformer_fixture(full, gfull, gfull16):
    """SURVEY 8 a7, fp16 variant: the reference's fp16-transformer export (use_fp16_transformer, Export_F5.py:20,88-89,139-140,
    198-199,321-326,348-349; F5/fp16/modules.py:467) run on torch-CPU fp16 at the BASELINE shapes -> tests/golden/f5_full_fp16.npz.
    Two f16 engines against it: the engine's own f16 form, and `ref_fp16_attn` (the export's attention rounding points: q / k
    with the extra x0.1 folded in before the fp16 rounding, q k scores rounded to fp16, x100 in fp32, fp32 softmax, fp16
    probabilities).  The reference chain rounds EVERY tensor to fp16 (residual stream and sampler state included), the engine
    keeps those in fp32, so the comparison is a distance, not an identity:
      * each engine is within 5e-4 waveform rms (of full scale) of the reference-fp16 waveform and its single DiT evaluation
        within 4e-3 relative rms of the reference-fp16 one (the reference's own fp16-vs-fp32 distances, measured when the
        fixture was written: 1.4e-4 and 1.6e-3);
      * each engine is no farther from the reference's FP32 chain than the reference's own fp16 chain is (x1.25 slack)."""
    import dataclasses
    cfg, raw, audio, ids, N, noise = full
    assert int(gfull16["N"]) == N and int(gfull16["ref_signal_len"]) == 563
    assert gfull16["dit_pred_t7"].dtype == np.float16 and gfull16["loop_final"].dtype == np.float16
    w16 = gfull16["e2e_i16"].astype(np.float64)
    w32 = gfull["e2e_i16"].astype(np.float64)
    ref_gap = rms((w16 - w32) / 32767.0)                               # the reference's own fp16-vs-fp32 distance
    ref_gap_pred = rms(gfull16["dit_pred_t7"].astype(np.float64) - gfull["dit_pred_t7"]) / rms(gfull["dit_pred_t7"])
    assert 5e-5 < ref_gap < 5e-4 and 5e-4 < ref_gap_pred < 5e-3, (ref_gap, ref_gap_pred)
    p16 = gfull16["dit_pred_t7"].astype(np.float64)
    for mode in (False, True):
        c = dataclasses.replace(cfg, ref_fp16_attn=mode)
        eng = F5Engine(c, raw, dtype="f16")
        o = eng.preprocess(audio[0].reshape(1, 1, -1), ids[0].reshape(1, -1), np.array([N]), noise=noise[0])
        pred = eng.dit_eval(noise[:1], o["cat_mel_text"], o["cat_mel_text_drop"], 7)
        e_pred16 = rms(pred - p16) / rms(p16)
        e_pred32 = rms(pred - gfull["dit_pred_t7"]) / rms(gfull["dit_pred_t7"])
        w = eng.synthesize(audio[:1], ids[:1], N, noise=noise[:1])[0, 0].astype(np.float64)
        e16 = rms((w - w16) / 32767.0)
        e32 = rms((w - w32) / 32767.0)
        eng.close()
        print(f"F5 full size f16 engine (ref_fp16_attn={mode}) vs reference fp16 export: DiT eval rel {e_pred16:.2e}, waveform rms "
              f"{e16:.2e}; vs reference fp32: DiT eval rel {e_pred32:.2e}, waveform rms {e32:.2e}  "
              f"[reference fp16 vs its fp32: {ref_gap_pred:.2e} / {ref_gap:.2e}]")
        assert e_pred16 < 4e-3 and e16 < 5e-4, (mode, e_pred16, e16)
        assert e_pred32 < 1.25 * ref_gap_pred and e32 < 1.25 * ref_gap, (mode, e_pred32, e32, ref_gap_pred, ref_gap)


def test_ref_fp16_attn_is_an_f16_only_form():
    import dataclasses
    cfg = dataclasses.replace(F5Config.small(), ref_fp16_attn=True)
    raw = W.synth_state(W.f5_spec(cfg), 9527)
    with pytest.raises(Exception, match="f16"):
        F5Engine(cfg, raw, dtype="f32")


def test_real_prompt_stft_and_mel(golden_dir, small):
    """G1: the first second of the real prompt IndexTTS/example/zh.wav through the engine's front end against
    the reference's STFT_Process (stft_B, STFT_Process.py:153-157) and the F5Preprocess mel (Export_F5.py:122-125)."""
    cfg, st, eng = small
    z = np.load(os.path.join(golden_dir, "zh_prompt.npz"))
    pcm = z["pcm"]
    assert int(z["total_samples"]) == 162240 and pcm.shape == (24000,)
    re, im = eng.stft(pcm)
    sc = float(np.abs(z["stft_re"]).max())
    assert re.shape == z["stft_re"].shape == (513, 94)
    assert np.abs(re - z["stft_re"]).max() < 2e-5 * max(sc, 1.0) and np.abs(im - z["stft_im"]).max() < 2e-5 * max(sc, 1.0)
    R = pcm.shape[0] // cfg.hop_length + 1
    o = eng.preprocess(pcm.reshape(1, 1, -1), np.zeros((1, 4), np.int32), np.array([R + 8]))
    lm = o["cat_mel_text"][0, :R, :100].T
    # log of a clamped magnitude: compare where the reference is above the clamp floor
    m = z["logmel"] > np.log(2e-5)
    assert m.mean() > 0.9
    assert np.abs(lm - z["logmel"])[m].max() < 2e-3


# ---------------------------------------------------------------------------------------------
# Round 4: the AdaLN fold, the engine-level fp32 arithmetic and the fp16-pair range watch
# ---------------------------------------------------------------------------------------------
def _mid_cfg(**kw):
    """Full-width DiT layers (dim 1024 / heads 16: the shapes whose kernels carry the fold), two blocks, small front / back end."""
    return F5Config(depth=2, text_dim=64, text_num_embeds=40, conv_layers=1, vocos_dim=64, vocos_intermediate=128, vocos_layers=1,
                    nfe_step=4, **kw)


def _mid_inputs(cfg, U, N, seed=3):
    noise = np.stack([W.synth_normal(seed + u, f"n{N}", (N, cfg.mel_dim)) for u in range(U)])
    cmt = np.stack([W.synth_normal(seed + 11 + u, f"c{N}", (N, cfg.mel_dim + cfg.text_dim), std=0.7) for u in range(U)])
    cmtd = np.stack([W.synth_normal(seed + 22 + u, f"d{N}", (N, cfg.mel_dim + cfg.text_dim), std=0.7) for u in range(U)])
    return noise, cmt, cmtd


def _norm_launches(eng, noise, cmt, cmtd, k):
    from mi355tts import _lib
    _lib.prof_reset(); _lib.prof_enable(["norm", "conv_gemm"])
    try:
        eng.dit_eval(noise, cmt, cmtd, k)
    finally:
        _lib.prof_enable(())
    ks = _lib.prof_kernels()
    return _lib.prof_get("norm")["launches"], [x["kernel"] for x in ks]


@pytest.mark.parametrize("dtype,tol_paths,tol_oracle", [("f32", 1e-6, 5e-6), ("f16", 5e-4, 1.5e-3), ("bf16", 4e-3, 1.2e-2)])      # achieved: 2.3e-7 / 1.4e-6, 1.4e-4 / 4.5e-4, 1.1e-3 / 3.6e-3
def test_adaln_fold_against_rownorm_path_and_oracle(dtype, tol_paths, tol_oracle):
    """AdaLayerNorm (modules.py:301-305) folded into the GEMM epilogues either side of it (gemm_epilogue.h): the O / FF2 epilogue
    leaves x o (1 + scale) and per-row partial statistics, the QKV / FF1 epilogue finishes rstd * acc - mean * rstd * W(1 + scale)
    + (W shift + b).  Against the same engine with the fold off (row-norm launches) and against the oracle; one and three
    utterances (the stream-K panel-plane kernel / the 128x128 and 256x256 16-bit kernels), odd and panel-filling token counts."""
    import dataclasses
    cfg = _mid_cfg()
    raw = W.synth_state(W.f5_spec(cfg), 7)
    st = W.fold_f5(cfg, raw)
    tables = O.time_tables(cfg, st)
    e_fold = F5Engine(cfg, raw, dtype=dtype)
    e_rows = F5Engine(dataclasses.replace(cfg, adaln_fold=False), raw, dtype=dtype)
    try:
        assert e_fold.info()["adaln_fold"] and not e_rows.info()["adaln_fold"]
        # (fp32: the panel-plane kernel takes a layer from 64 tiles of 128 x 128 on: >= 897 rows for the O / FF2 projections)
        for U, N in ((1, 500), (3, 257), (2, 640)) if dtype == "f32" else ((1, 300), (3, 257), (8, 1126)):
            noise, cmt, cmtd = _mid_inputs(cfg, U, N)
            a = e_fold.dit_eval(noise, cmt, cmtd, 2)
            b = e_rows.dit_eval(noise, cmt, cmtd, 2)
            e_ab = rms(a - b) / rms(b)
            assert np.isfinite(a).all() and e_ab < tol_paths, (dtype, U, N, e_ab)
            n_fold, names = _norm_launches(e_fold, noise, cmt, cmtd, 2)
            n_rows, _ = _norm_launches(e_rows, noise, cmt, cmtd, 2)
            # the fold keeps two norm-family launches per evaluation (the first block's prologue, AdaLN-final) — plus, in the 16-bit
            # engines, one tiny ln_finalize launch per norm; rows: 2 row-norm launches per block + 1
            assert n_fold == (2 if dtype == "f32" else 2 + 2 * cfg.depth) and n_rows == 2 * cfg.depth + 1, (n_fold, n_rows, names)
            assert not any("rownorm_x3p" in k for k in names)
            if dtype == "f32":
                assert any("AdaLN fold" in k for k in names), names
            if U <= 3:
                cos, sin = O.rope_tables(N, 64)
                ref = O.dit_forward(cfg, st, noise[0], cmt[0], cmtd[0], tables[2][2], cos, sin)
                e_o = rms(a[:2] - ref) / rms(ref)
                assert e_o < tol_oracle, (dtype, U, N, e_o)
                print(f"AdaLN fold {dtype} U={U} N={N}: fold vs row-norm path rel rms {e_ab:.2e}, fold vs oracle {e_o:.2e}")
        # run-to-run identity of the fold (plain stores, fixed summation order everywhere)
        a2 = e_fold.dit_eval(noise, cmt, cmtd, 2)
        assert np.array_equal(a, a2)
    finally:
        e_fold.close(); e_rows.close()


@pytest.mark.parametrize("offset", [20.0, 100.0])
def test_adaln_fold_rows_with_a_dc_offset(offset):
    """nn.LayerNorm is two-pass; the fold's row statistics were E[x^2] - mean^2 over fp32 partial sums, whose cancellation
    error grows as eps * mean^2 / var — invisible on the synthetic weights (row means ~ 0).  The statistics now travel as (sum, M2
    about the block mean) pairs merged Chan-style (wave_reduce.h).  Here the residual stream carries a common offset of `offset`
    standard deviations (input_embed.proj.bias shifted): the fold must still agree with the row-norm path and the oracle.  (At
    offset 100 the old formula's variance error alone was 6e-8 * 1e4 = 6e-4.)"""
    import dataclasses
    cfg = _mid_cfg()
    raw = dict(W.synth_state(W.f5_spec(cfg), 7))
    raw["transformer.input_embed.proj.bias"] = raw["transformer.input_embed.proj.bias"] + np.float32(offset)
    st = W.fold_f5(cfg, raw)
    tables = O.time_tables(cfg, st)
    e_fold = F5Engine(cfg, raw, dtype="f32")
    e_rows = F5Engine(dataclasses.replace(cfg, adaln_fold=False), raw, dtype="f32")
    try:
        U, N = 1, 500
        noise, cmt, cmtd = _mid_inputs(cfg, U, N)
        a = e_fold.dit_eval(noise, cmt, cmtd, 2)
        b = e_rows.dit_eval(noise, cmt, cmtd, 2)
        cos, sin = O.rope_tables(N, 64)
        ref = O.dit_forward(cfg, st, noise[0], cmt[0], cmtd[0], tables[2][2], cos, sin)
        e_ab, e_ao, e_bo = rms(a - b) / rms(b), rms(a[:2] - ref) / rms(ref), rms(b[:2] - ref) / rms(ref)
        print(f"AdaLN fold with a DC offset of {offset}: fold vs row-norm {e_ab:.2e}, fold vs oracle {e_ao:.2e}, row-norm vs oracle {e_bo:.2e}")
        assert np.isfinite(a).all() and e_fold.info()["saturation_events"] == 0
        # what remains is the fold's own rounding: operands rounded relative to |x| (22 bits) instead of |x - mean|
        assert e_ab < 2e-7 * max(offset, 10.0) and e_ao < 2e-7 * max(offset, 10.0) + 5e-6, (offset, e_ab, e_ao, e_bo)
    finally:
        e_fold.close(); e_rows.close()


def test_two_engines_with_different_fp32_arithmetic_coexist():
    """The fp32 arithmetic is a property of the engine (F5Config.f32_arithmetic), not of the process: an fp16-pair engine, a
    three-plane bf16 engine and a native-fp32-MFMA engine alive at once, called alternately, each give exactly what they give
    alone — and report what they run (mi_f5_info)."""
    import dataclasses
    cfg = _mid_cfg()
    raw = W.synth_state(W.f5_spec(cfg), 7)
    noise, cmt, cmtd = _mid_inputs(cfg, 1, 500)
    kinds = ["fp16x2-pairs", "bf16x3", "native-fp32-mfma"]
    alone = {}
    for kind in kinds:
        e = F5Engine(dataclasses.replace(cfg, f32_arithmetic=kind), raw, dtype="f32")
        assert e.info()["f32_arithmetic"] == kind
        alone[kind] = e.dit_eval(noise, cmt, cmtd, 1)
        e.close()
    engines = {kind: F5Engine(dataclasses.replace(cfg, f32_arithmetic=kind), raw, dtype="f32") for kind in kinds}
    try:
        for _ in range(2):
            for kind in kinds:
                got = engines[kind].dit_eval(noise, cmt, cmtd, 1)
                assert np.array_equal(got, alone[kind]), kind
        assert not np.array_equal(alone["fp16x2-pairs"], alone["native-fp32-mfma"])
        for kind in kinds[:2]:
            assert rms(alone[kind] - alone["native-fp32-mfma"]) / rms(alone["native-fp32-mfma"]) < 3e-6
        assert F5Engine(cfg, raw, dtype="bf16").info()["f32_arithmetic"] is None
    finally:
        for e in engines.values():
            e.close()


def test_fp16_pair_range_watch_heavy_tailed_operands():
    """fp16 pairs hold |a| <= 65504 and used to clamp silently.  (a) activations: a DiT whose residual
    stream carries a few 1e5 outliers (a conditioning row scaled up) — the pair engine must notice (saturation_events), switch
    itself to the exact three-plane bf16 split, re-run the call, and agree with the native-fp32 engine; (b) weights: a matrix
    with one 1e5 entry is loaded straight into the three-plane format."""
    import dataclasses
    cfg = _mid_cfg()
    raw = W.synth_state(W.f5_spec(cfg), 7)
    noise, cmt, cmtd = _mid_inputs(cfg, 1, 500)
    e_nat = F5Engine(dataclasses.replace(cfg, f32_arithmetic="native-fp32-mfma"), raw, dtype="f32")
    e_pair = F5Engine(dataclasses.replace(cfg, f32_arithmetic="fp16x2-pairs"), raw, dtype="f32")
    try:
        ok = e_pair.dit_eval(noise, cmt, cmtd, 1)
        assert e_pair.info() == {"f32_arithmetic": "fp16x2-pairs", "saturation_events": 0, "adaln_fold": True}
        ref_ok = e_nat.dit_eval(noise, cmt, cmtd, 1)
        assert rms(ok - ref_ok) / rms(ref_ok) < 3e-6
        # heavy tail: 0.1 % of the conditioning entries at +-3e6 (they reach the residual stream through in_proj: rows of ~1e5)
        hot = cmt.copy()
        idx = np.unravel_index(np.arange(0, hot.size, 997), hot.shape)
        hot[idx] = 3e6 * np.sign(hot[idx] + 1e-9)
        ref = e_nat.dit_eval(noise, hot, cmtd, 1)
        got = e_pair.dit_eval(noise, hot, cmtd, 1)
        info = e_pair.info()
        assert info["saturation_events"] == 1 and info["f32_arithmetic"] == "bf16x3", info
        assert np.isfinite(got).all() and rms(got - ref) / rms(ref) < 1e-5, rms(got - ref) / rms(ref)
        # the switch is permanent and the ordinary input still gives an fp32-equivalent answer
        again = e_pair.dit_eval(noise, cmt, cmtd, 1)
        assert rms(again - ref_ok) / rms(ref_ok) < 3e-6 and e_pair.info()["saturation_events"] == 1
    finally:
        e_nat.close(); e_pair.close()
    big = {k: v.copy() for k, v in raw.items()}
    name = next(k for k in big if k.endswith("attn.to_q.weight"))
    big[name][3, 5] = 1e6          # (the q rows are folded with 64^-0.25 on the way in: still beyond 65504)
    e = F5Engine(dataclasses.replace(cfg, f32_arithmetic="fp16x2-pairs"), big, dtype="f32")
    try:
        assert e.info()["f32_arithmetic"] == "bf16x3"
        en = F5Engine(dataclasses.replace(cfg, f32_arithmetic="native-fp32-mfma"), big, dtype="f32")
        a, b = e.dit_eval(noise, cmt, cmtd, 1), en.dit_eval(noise, cmt, cmtd, 1)
        en.close()
        assert np.isfinite(a).all() and rms(a - b) / rms(b) < 1e-5
    finally:
        e.close()


def test_f16_adaln_fold_range_watch_falls_back_to_the_row_norm_path():
    """an f16 engine's AdaLN fold multiplies the UNNORMALISED residual row o (1 + scale) — not bounded by the norm like
    LN(x)(1 + scale) + shift.  A residual column pushed beyond 65504 (an output bias of 1e7 in block 0's O projection: biases and
    the residual stream are fp32 in every engine) must raise the engine's flag (gemm_epilogue_resid_ln: f16_range_word), the call
    is re-run with the fold off for that engine (capi.hip f5_run_checked), permanently, and the answer agrees with an engine that
    never folded.  The unmodified weights leave the fold on."""
    import dataclasses
    cfg = _mid_cfg()
    raw = W.synth_state(W.f5_spec(cfg), 7)
    noise, cmt, cmtd = _mid_inputs(cfg, 1, 500)
    hot = {k: v.copy() for k, v in raw.items()}
    hot["transformer.transformer_blocks.0.attn.to_out.0.bias"][5] = 1e7
    e_plain = F5Engine(dataclasses.replace(cfg, adaln_fold=True), raw, dtype="f16")
    e_fold = F5Engine(dataclasses.replace(cfg, adaln_fold=True), hot, dtype="f16")
    e_rows = F5Engine(dataclasses.replace(cfg, adaln_fold=False), hot, dtype="f16")
    try:
        e_plain.dit_eval(noise, cmt, cmtd, 1)
        assert e_plain.info()["adaln_fold"] is True and e_plain.info()["saturation_events"] == 0
        assert e_fold.info()["adaln_fold"] is True and e_rows.info()["adaln_fold"] is False
        got, ref = e_fold.dit_eval(noise, cmt, cmtd, 1), e_rows.dit_eval(noise, cmt, cmtd, 1)
        info = e_fold.info()
        assert info["saturation_events"] == 1 and info["adaln_fold"] is False, info
        assert np.isfinite(ref).all() and np.isfinite(got).all() and rms(got - ref) <= 1e-6 * rms(ref), rms(got - ref) / rms(ref)
        again = e_fold.dit_eval(noise, cmt, cmtd, 1)                         # permanent: no second event, same answer
        assert np.array_equal(again, got) and e_fold.info()["saturation_events"] == 1
    finally:
        e_plain.close(); e_fold.close(); e_rows.close()


def test_bigvgan_type_mel_front_end_against_reference_fixture(golden_dir):
    """The prompt features of the F5 *_bigvgan checkpoints (VERDICT r3 missing #1): get_bigvgan_mel_spectrogram
    (modeling_modified/F5/modules.py:30-72 — librosa/slaney mel basis, reflect pad (n_fft - hop) / 2, center=False,
    sqrt(re^2 + im^2 + 1e-9), log(clamp(., 1e-5))) selected by F5Config.mel_spec_type = "bigvgan", against the output of the
    reference function itself (tests/golden/make_golden_bigvgan_mel.py) and against the oracle's restatement."""
    import dataclasses
    cfg = dataclasses.replace(F5Config.small(), mel_spec_type="bigvgan")
    raw = W.synth_state(W.f5_spec(cfg), 9527)
    eng = F5Engine(cfg, raw, dtype="f32")
    g = np.load(os.path.join(golden_dir, "f5_bigvgan_mel.npz"))
    try:
        for name in ("syn", "zh"):
            pcm, ref = g[name + "_pcm"], g[name + "_logmel"].T            # (frames, 100)
            R = cfg.ref_frames(pcm.shape[0])
            assert R == ref.shape[0]
            o = eng.preprocess(pcm.reshape(1, 1, -1), np.zeros((1, 4), np.int32), np.array([R + 8]))
            assert int(o["ref_signal_len"]) == R
            lm = o["cat_mel_text"][0, :R, :100]
            assert np.all(o["cat_mel_text"][0, R:, :100] == 0.0)
            m = ref > np.log(2e-5)                                        # log of a clamped value: compare above the clamp floor
            assert m.mean() > 0.6
            err = np.abs(lm - ref)[m].max()
            orc = O.bigvgan_mel(pcm.astype(np.float32) * np.float32(1.0 / 32768.0))
            print(f"bigvgan-type mel ({name}): max |log-mel - reference| above the floor {err:.2e}; oracle vs reference {np.abs(orc - ref)[m].max():.2e}")
            assert err < (1e-4 if name == "syn" else 5e-4), err            # zh.wav: near-silent frames sit close to the floor (oracle: 1.7e-4)
    finally:
        eng.close()
    # the vocos-type default is untouched: other frame count for the same audio
    assert F5Config().ref_frames(144000) == 563 and dataclasses.replace(F5Config(), mel_spec_type="bigvgan").ref_frames(144000) == 562
