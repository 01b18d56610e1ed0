"""GPU parity: the HIP BigVGAN path (through the C-ABI) against the numpy oracle and the golden
vectors generated from the reference's own module code.

Tolerances
  fp32: the engine uses exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) with fp32 accumulation, so the only
        differences to the oracle are summation order: <= 2e-5 abs on O(1) activations, and the
        north-star bound (waveform RMS error <= 1e-3) is asserted with 100x headroom.
  fp16: storage is rounded to fp16 after every layer (like the reference's whole-graph fp16 cast,
        BigVGAN/Optimize_ONNX.py:67-74); bound = 2e-2 RMS on the [-1,1] waveform.
"""
import os

import numpy as np
import pytest

from mi355tts.config import BigVGANConfig
from mi355tts import weights as W
from mi355tts import bigvgan as BV
from oracle import bigvgan_np as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "bigvgan_small.npz"))


def rms(a):
    return float(np.sqrt(np.mean(np.square(a.astype(np.float64)))))


# ---------------------------------------------------------------------------------------------
# K-CONV1D / K-CONVT (implicit-GEMM MFMA kernel)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ci,Co,k,d,T,B", [
    (24, 24, 3, 1, 300, 2), (24, 24, 11, 5, 517, 1), (48, 48, 7, 3, 260, 1), (96, 96, 3, 5, 129, 2),
    (192, 192, 7, 1, 140, 1), (768, 768, 11, 3, 70, 1), (100, 1536, 7, 1, 33, 2), (8, 16, 3, 1, 5, 1),
    (16, 40, 5, 2, 1, 1),
])
def test_conv1d_f32(Ci, Co, k, d, T, B):
    x = W.synth_normal(1, f"x{Ci}{k}{d}", (B, Ci, T))
    w = W.synth_normal(2, f"w{Ci}{k}{d}", (Co, Ci, k), std=1.0 / np.sqrt(Ci * k))
    b = W.synth_normal(3, "b", (Co,), std=0.1)
    pad = (k * d - d) // 2
    ref = O.conv1d(x, w, b, dilation=d, padding=pad)
    y = BV.conv1d(x, w, b, dilation=d, padding=pad)
    assert y.shape == ref.shape
    np.testing.assert_allclose(y, ref, atol=2e-5, rtol=1e-5)


def test_conv1d_is_transpose_detecting():
    # asymmetric weights + A = shifted identity: a swapped row/col mapping cannot pass
    Ci = Co = 32
    T = 64
    x = np.zeros((1, Ci, T), np.float32)
    x[0, np.arange(Ci), np.arange(Ci) + 3] = 1.0
    w = (np.arange(Co * Ci * 3, dtype=np.float32).reshape(Co, Ci, 3) % 17) / 17.0
    ref = O.conv1d(x, w, None, padding=1)
    y = BV.conv1d(x, w, None, padding=1)
    np.testing.assert_allclose(y, ref, atol=1e-6)


@pytest.mark.parametrize("dtype,tol", [("f16", 6e-3), ("bf16", 4e-2)])
def test_conv1d_lowp(dtype, tol):
    x = W.synth_normal(1, "xl", (2, 96, 200))
    w = W.synth_normal(2, "wl", (96, 96, 7), std=1.0 / np.sqrt(96 * 7))
    b = W.synth_normal(3, "bl", (96,), std=0.1)
    ref = O.conv1d(x, w, b, dilation=3, padding=9)
    y = BV.conv1d(x, w, b, dilation=3, padding=9, dtype=dtype)
    assert rms(y - ref) / rms(ref) < tol


def test_grouped_conv1d_f32():
    # the F5 conv-position-embedding shape: 1024 ch, 16 groups, k31 (modules.py:167-190), shortened
    C, G, k, T = 256, 4, 31, 90
    x = W.synth_normal(1, "xg", (2, C, T))
    w = W.synth_normal(2, "wg", (C, C // G, k), std=1.0 / np.sqrt(C // G * k))
    b = W.synth_normal(3, "bg", (C,), std=0.1)
    ref = np.concatenate([O.conv1d(x[:, g * (C // G):(g + 1) * (C // G)], w[g * (C // G):(g + 1) * (C // G)],
                                   b[g * (C // G):(g + 1) * (C // G)], padding=15) for g in range(G)], axis=1)
    y = BV.conv1d(x, w, b, padding=15, groups=G)
    np.testing.assert_allclose(y, ref, atol=2e-5, rtol=1e-5)


@pytest.mark.parametrize("Ci,Co,u,T,B", [(1536, 768, 4, 20, 1), (96, 48, 2, 301, 2), (48, 24, 2, 257, 1), (16, 8, 4, 1, 1)])
def test_conv_transpose1d_f32(Ci, Co, u, T, B):
    x = W.synth_normal(1, f"xt{Ci}", (B, Ci, T))
    w = W.synth_normal(2, f"wt{Ci}", (Ci, Co, 2 * u), std=1.0 / np.sqrt(2 * Ci))
    b = W.synth_normal(3, "bt", (Co,), std=0.1)
    ref = O.conv_transpose1d(x, w, b, stride=u, padding=u // 2)
    y = BV.conv_transpose1d(x, w, b, stride=u, padding=u // 2)
    assert y.shape == ref.shape == (B, Co, T * u)
    np.testing.assert_allclose(y, ref, atol=2e-5, rtol=1e-5)


def test_conv_transpose_rejects_unsupported():
    from mi355tts._lib import MiError
    x = np.zeros((1, 8, 4), np.float32)
    with pytest.raises(MiError):
        BV.conv_transpose1d(x, np.zeros((8, 8, 3), np.float32), None, stride=1, padding=1)


# ---------------------------------------------------------------------------------------------
# K-AA (fused anti-aliased SnakeBeta)
# ---------------------------------------------------------------------------------------------
def test_aa_golden_block_and_post(g):
    y = BV.aa_activation1d(g["act_x"], g["act_alpha"], g["act_beta"])
    np.testing.assert_allclose(y, g["act_y"], atol=1e-5)
    yp = BV.aa_activation1d(g["post_x"], g["post_alpha"], g["post_beta"], post=True)
    assert yp.shape[-1] == g["post_x"].shape[-1] + 30
    np.testing.assert_allclose(yp, g["post_y"], atol=1e-5)


@pytest.mark.parametrize("C,T,B", [(24, 1000, 2), (48, 333, 1), (96, 41, 1), (192, 70, 2), (768, 9, 1), (24, 1, 1), (8, 7, 3)])
@pytest.mark.parametrize("post", [False, True])
def test_aa_vs_oracle_f32(C, T, B, post):
    x = W.synth_normal(5, f"aa{C}{T}", (B, C, T), std=1.5)
    a = W.synth_normal(6, "a", (C,), std=0.3)
    b = W.synth_normal(7, "b", (C,), std=0.3)
    ref = O.activation1d(x, a, b, O.aa_filter(), post=post)
    y = BV.aa_activation1d(x, a, b, post=post)
    assert y.shape == ref.shape
    np.testing.assert_allclose(y, ref, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("C,k,d,T,B", [(24, 3, 1, 700, 2), (24, 11, 5, 300, 1), (48, 7, 3, 515, 2), (96, 11, 5, 260, 1), (96, 3, 1, 130, 2),
                                       (16, 7, 1, 40, 1), (8, 3, 1, 5, 3)])
@pytest.mark.parametrize("with_res", [False, True])
def test_fused_aa_conv_vs_oracle_f32(C, k, d, T, B, with_res):
    """The fused kernel of the low-channel stages alone (`xt = c(a(x))`, `x = c2(a2(xt)) + x`: one half of an AMPBlock1
    iteration, bigvgan.py:132-140): tile halos across ragged T, every (k, dilation) of the model, residual on / off."""
    x = W.synth_normal(5, f"ac{C}{T}", (B, C, T), std=1.5)
    a = W.synth_normal(6, "a", (C,), std=0.3)
    b = W.synth_normal(7, "b", (C,), std=0.3)
    w = W.synth_normal(8, f"w{C}{k}", (C, C, k), std=1.0 / np.sqrt(C * k))
    bias = W.synth_normal(9, "bias", (C,), std=0.1)
    res = W.synth_normal(10, f"r{C}{T}", (B, C, T)) if with_res else None
    ref = O.conv1d(O.activation1d(x, a, b, O.aa_filter()), w, bias, dilation=d, padding=O.get_padding(k, d))
    if with_res:
        ref = ref + res
    y = BV.aa_conv1d(x, a, b, w, bias, dilation=d, res=res)
    assert y.shape == ref.shape
    np.testing.assert_allclose(y, ref, atol=3e-5, rtol=1e-5)


def test_amp_block_golden_through_fused_kernels(g, small_voc):
    """G8a: the three AMPBlock1 of the reference (BigVGAN/modeling_modified/bigvgan.py:132-140, k = 3 / 7 / 11, dilations 1,3,5)
    rebuilt from six fused AA+conv launches each, against the reference's own block outputs `amp_y*`."""
    cfg, st, v = small_voc
    x = g["amp_x"]
    for j, k in enumerate(cfg.resblock_kernel_sizes):
        cur = x
        for l, d in enumerate(cfg.resblock_dilation_sizes[j]):
            p = f"resblocks.{j}."
            t = BV.aa_conv1d(cur, st[p + f"activations.{2 * l}.act.alpha"], st[p + f"activations.{2 * l}.act.beta"],
                             st[p + f"convs1.{l}.weight"], st[p + f"convs1.{l}.bias"], dilation=d)
            cur = BV.aa_conv1d(t, st[p + f"activations.{2 * l + 1}.act.alpha"], st[p + f"activations.{2 * l + 1}.act.beta"],
                               st[p + f"convs2.{l}.weight"], st[p + f"convs2.{l}.bias"], dilation=1, res=cur)
        np.testing.assert_allclose(cur, g[f"amp_y{j}"], atol=3e-5)


def test_aa_f16_storage():
    x = W.synth_normal(5, "aah", (2, 48, 500), std=1.5)
    a = W.synth_normal(6, "a", (48,), std=0.3)
    b = W.synth_normal(7, "b", (48,), std=0.3)
    ref = O.activation1d(x, a, b, O.aa_filter())
    y = BV.aa_activation1d(x, a, b, dtype="f16")
    assert rms(y - ref) / rms(ref) < 2e-3


# ---------------------------------------------------------------------------------------------
# whole generator
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_voc():
    cfg = BigVGANConfig.small()
    st = W.synth_state(W.bigvgan_spec(cfg), 9527)
    v = BV.BigVGANVocoder(cfg, st, dtype="f32")
    yield cfg, st, v
    v.close()


@pytest.mark.parametrize("name", ["a", "b", "ones"])
def test_generator_golden_small(g, small_voc, name):
    cfg, st, v = small_voc
    mel = g[f"gen_mel_{name}"]
    w = v.run(mel)
    assert w.dtype == np.int16 and w.shape == (mel.shape[0], 1, cfg.out_len(mel.shape[2]))
    assert np.abs(w.astype(np.int32) - g[f"gen_i16_{name}"].astype(np.int32)).max() <= 1
    if name != "ones":
        y = v.run_float(mel)
        np.testing.assert_allclose(y, g[f"gen_y_{name}"], atol=2e-5)


@pytest.fixture(scope="module")
def full_state():
    cfg = BigVGANConfig()
    return cfg, W.synth_state(W.bigvgan_spec(cfg), 9527)


def _mel(B, F, seed=11):
    return W.synth_normal(seed, "mel", (B, 100, F), std=2.0, mean=-2.0).clip(-11.5, 2.5)


def test_generator_full_arch_f32(full_state):
    cfg, st = full_state
    v = BV.BigVGANVocoder(cfg, st, dtype="f32")
    mel = _mel(2, 12)
    ref = O.generator(cfg, st, mel)
    y = v.run_float(mel)
    assert y.shape == ref.shape == (2, 1, 12 * 256 + 30)
    err = rms(y - ref)
    assert err < 1e-5, err                       # north-star bound is 1e-3
    wi = v.run(mel)
    wr = O.bigvgan_int16(cfg, st, mel)
    assert np.abs(wi.astype(np.int32) - wr.astype(np.int32)).max() <= 2
    # batch independence (the B>1 extension must equal the reference's batch-1 graph per item)
    y0 = v.run_float(mel[1:2])
    assert np.array_equal(y0[0], y[1])
    v.close()


def test_generator_full_arch_f16(full_state):
    cfg, st = full_state
    v = BV.BigVGANVocoder(cfg, st, dtype="f16")
    mel = _mel(1, 12)
    ref = O.generator(cfg, st, mel)
    y = v.run_float(mel)
    err = rms(y - ref)
    assert err < 2e-2, err
    assert rms(ref) > 0.05                       # the comparison is not vacuous
    v.close()


def test_full_size_properties(full_state):
    """BASELINE config[0] size (1,100,512): length, range, determinism, torch zero-copy path."""
    import torch
    cfg, st = full_state
    v = BV.BigVGANVocoder(cfg, st, dtype="f16")
    mel = _mel(1, 512)
    w1 = v.run(mel)
    assert w1.shape == (1, 1, 131102)
    assert np.array_equal(w1, v.run(mel))
    assert 500 < rms(w1) < 30000
    wt = v.run_torch(torch.from_numpy(mel).cuda())
    assert np.array_equal(wt.cpu().numpy(), w1)
    # time-shift consistency away from the edges: the generator is a (zero-padded) convolutional map
    mel2 = np.concatenate([_mel(1, 4, seed=3), mel[:, :, :-4]], axis=2)
    w2 = v.run(mel2)
    a = w1[0, 0, 64 * 256:300 * 256].astype(np.int32)
    b = w2[0, 0, 68 * 256:304 * 256].astype(np.int32)
    assert np.abs(a - b).max() <= 64             # fp16 tile-boundary rounding only
    v.close()


@pytest.mark.parametrize("dtype,B,F", [("f32", 2, 24), ("f16", 3, 40), ("bf16", 1, 33)])
def test_amp_blocks_on_side_streams_are_bit_identical(full_state, dtype, B, F):
    """The three AMP blocks of a stage (resblock kernels 3 / 7 / 11, bigvgan.py:384-398) only meet in their input and in the
    accumulation of their outputs; by default (bigvgan_streams = 3) blocks 1 and 2 run on side streams of the handle with
    scratch of their own and the accumulation keeps its block order through events.  Same kernels, same order of every
    rounding: the waveform must equal the one-stream forward bit for bit, in every stream mode, run after run."""
    from mi355tts import _lib
    cfg, st = full_state
    v = BV.BigVGANVocoder(cfg, st, dtype=dtype)
    mel = _mel(B, F, seed=23)
    saved = _lib.get_option("bigvgan_streams")
    try:
        _lib.set_option("bigvgan_streams", 1)
        ref = v.run(mel)
        assert rms(ref) > 100
        for ns in (2, 3, 3, 1):
            _lib.set_option("bigvgan_streams", ns)
            assert np.array_equal(v.run(mel), ref), ns
    finally:
        _lib.set_option("bigvgan_streams", saved)
        v.close()


def test_full_size_reference_fixture(full_state, golden_dir):
    """BASELINE configs[0] / [1] against the REFERENCE generator + int16 wrapper run at the real shape
    (tests/golden/make_golden_full.py: BigVGAN/modeling_modified/bigvgan.py:384-410 through Export_BigVGAN.py:37-49 on
    mel (1,100,512)).  fp32: the north-star gate (1e-3 RMS) with headroom + int16 within the truncation boundary;
    fp16 B=8 (configs[1]): item 0 of the bench batch is the fixture's mel, the same mel tiled 8 times must give 8 equal
    waveforms, gate 4e-3 RMS (achieved 6.3e-4; storage rounded to fp16 after every layer)."""
    cfg, st = full_state
    gf = np.load(os.path.join(golden_dir, "bigvgan_full.npz"))
    ref = gf["wav_i16"].astype(np.float64)
    assert ref.shape == (131102,) and rms(ref) > 1000
    mel8 = W.bigvgan_synthetic_mel(cfg, 8, 512, 0)
    v = BV.BigVGANVocoder(cfg, st, dtype="f32")
    w = v.run(mel8[:1])
    d = np.abs(w[0, 0].astype(np.int32) - gf["wav_i16"].astype(np.int32))
    err32 = rms((w[0, 0] - ref) / 32767.0)
    assert err32 < 1e-4, err32                                       # north-star gate 1e-3
    assert d.max() <= 4 and (d > 1).mean() < 1e-3, (d.max(), (d > 1).mean())
    ones = v.run(np.ones((1, cfg.num_mels, 64), np.float32))       # the reference's own smoke input (Export_BigVGAN.py:165)
    assert np.abs(ones[0, 0].astype(np.int32) - gf["ones64_i16"].astype(np.int32)).max() <= 2
    v.close()
    v = BV.BigVGANVocoder(cfg, st, dtype="f16")
    w8 = v.run(mel8)
    assert w8.shape == (8, 1, 131102)
    err16 = rms((w8[0, 0] - ref) / 32767.0)
    assert err16 < 4e-3, err16                                       # achieved 6.3e-4 (profiles/r3); stated bound of the fp16 form 2e-2
    # batch position does not change an item's result, and neither does running it again: bit-identical in the DEFAULT
    # policy (two workgroups of the fused AA+conv kernel per CU).  Round 2 tolerated <= 64 LSB here; the cause was one
    # sample per channel read through `v_pk_fma_f32 ... op_sel:[0,1,0]` next to another workgroup's MFMAs (aa_math.h,
    # profiles/r3/aa_conv_opsel_*.txt) and is gone with the channel-pair form of the AA math.
    tiled = np.repeat(mel8[:1], 8, axis=0)
    wt = v.run(tiled)
    for b in range(8):
        assert np.array_equal(wt[b], wt[0]), (b, np.abs(wt[b, 0].astype(np.int32) - wt[0, 0].astype(np.int32)).max())
    for _ in range(3):
        assert np.array_equal(wt, v.run(tiled))
    assert np.array_equal(wt[0], w8[0])
    v.close()
    print(f"BigVGAN full size vs reference: fp32 rms {err32:.2e} (max |d| {d.max()} LSB), fp16 B=8 rms {err16:.2e}")


def test_bad_inputs_raise(small_voc):
    cfg, st, v = small_voc
    with pytest.raises(ValueError):
        v.run(np.zeros((1, cfg.num_mels + 1, 4), np.float32))
    with pytest.raises(ValueError):
        v.run(np.zeros((1, cfg.num_mels, 0), np.float32))
    from mi355tts._lib import MiError
    with pytest.raises(MiError):
        BV.BigVGANVocoder(cfg, blob=np.zeros(10, np.float32))


# ---------------------------------------------------------------------------------------------
# every tile configuration of the 16-bit LDS-DMA GEMM, forced at test sizes (they normally engage
# only when the launch fills the chip) and compared with the oracle
# ---------------------------------------------------------------------------------------------
@pytest.fixture
def gemm_options():
    """set_option for a test; every key it set goes back to the value it had before."""
    from mi355tts import _lib
    saved = {}

    def set_option(key, value):
        saved.setdefault(key, _lib.get_option(key))
        _lib.set_option(key, value)
    yield set_option
    for k, v in saved.items():
        _lib.set_option(k, v)


@pytest.mark.parametrize("cfg_name,opts,Ci,Co,k,d,T,B", [
    ("256x256/2-stage", {"gemm_big_tile_min": 1, "gemm_dma3_k_min": 0}, 768, 768, 7, 3, 700, 2),
    ("256x256/2-stage ragged N", {"gemm_big_tile_min": 1, "gemm_dma3_k_min": 0}, 256, 1000, 3, 1, 333, 1),
    ("256x192/2-stage", {"gemm_n192_min": 1}, 192, 192, 11, 5, 900, 2),
    ("256x192/2-stage N=384", {"gemm_n192_min": 1}, 384, 384, 3, 1, 515, 1),
    ("256x128/3-stage", {"gemm_big_tiles": 0, "gemm_n192": 0, "gemm_mid_tile_min": 1, "gemm_dma3_k_min": 0}, 384, 384, 7, 1, 600, 2),
    ("128x128/2-stage dma", {"gemm_use_dma3": 0, "gemm_ring4": 0, "gemm_small16_max": 0}, 768, 768, 3, 1, 300, 1),
    ("128x128/4-stage ring", {"gemm_use_dma3": 0, "gemm_small16_max": 0}, 768, 768, 3, 1, 300, 1),
    ("128x128/4-stage ring, Cin tail, ragged", {"gemm_use_dma3": 0, "gemm_small16_max": 0}, 200, 300, 7, 2, 333, 2),
    ("64x64 tiles (16-bit, few tiles)", {"gemm_use_dma3": 0}, 768, 768, 3, 1, 300, 1),
    ("64x64 tiles, Cin tail, ragged", {"gemm_use_dma3": 0}, 200, 300, 7, 2, 333, 2),
    ("128x128/2-stage dma (many tiles)", {"gemm_use_dma3": 0, "gemm_ring4_max": 4, "gemm_small16_max": 0}, 768, 768, 3, 1, 300, 1),
    ("128x128 flat-address DMA (no buffer descriptors)", {"gemm_use_dma3": 0, "gemm_buf": 0, "gemm_small16_max": 0}, 768, 768, 3, 1, 300, 1),
    ("128x128 ring, flat-address DMA", {"gemm_use_dma3": 0, "gemm_buf": 0, "gemm_ring4_max": 4096, "gemm_small16_max": 0}, 768, 768, 7, 3, 600, 2),
    ("256-row tiles need whole chunks: Cin = 200 falls back", {"gemm_big_tile_min": 1, "gemm_dma3_k_min": 0}, 200, 768, 7, 1, 700, 2),
    ("register-staged", {"gemm_use_dma3": 0, "gemm_use_dma": 0}, 192, 192, 7, 3, 300, 1),
])
@pytest.mark.parametrize("dtype,tol", [("f16", 6e-3), ("bf16", 4e-2)])
def test_gemm_tile_configs_vs_oracle(gemm_options, cfg_name, opts, Ci, Co, k, d, T, B, dtype, tol):
    for key, v in opts.items():
        gemm_options(key, v)
    x = W.synth_normal(21, f"tx{Ci}{k}", (B, Ci, T))
    w = W.synth_normal(22, f"tw{Ci}{Co}{k}", (Co, Ci, k), std=1.0 / np.sqrt(Ci * k))
    b = W.synth_normal(23, "tb", (Co,), std=0.1)
    pad = (k * d - d) // 2
    ref = O.conv1d(x, w, b, dilation=d, padding=pad)
    y = BV.conv1d(x, w, b, dilation=d, padding=pad, dtype=dtype)
    assert y.shape == ref.shape
    assert rms(y - ref) / rms(ref) < tol, cfg_name
    # element-wise too (a transposed or shifted tile would pass an RMS-of-noise check only by accident)
    assert np.abs(y - ref).max() < 40 * tol * rms(ref), cfg_name


@pytest.mark.parametrize("dtype,tol", [("f32", 0.0), ("f16", 6e-3), ("bf16", 4e-2)])
@pytest.mark.parametrize("stages", [0, 2, 3, 4])
@pytest.mark.parametrize("Ci,Co,T,B", [(256, 1000, 1500, 1), (512, 1024, 1126, 2), (128, 3072, 700, 2), (1024, 1024, 1126, 2),
                                        (256, 2048, 2252, 1), (128, 1280, 4000, 1)])
def test_stream_k_linear_vs_oracle(gemm_options, dtype, tol, stages, Ci, Co, T, B):
    """gemm_sk.hip: persistent workgroups over equal (tile, K chunk) ranges; tiles split between workgroups are summed in range
    order by the owner of the tile's first chunk.  Ragged M / N tails, every ring depth, partial tiles of 2..many pieces, and
    bit-identical results from run to run (the fix-up order is fixed).  The last two shapes have more tiles than persistent
    workgroups (288 / 320 tiles)."""
    gemm_options("gemm_sk", 2)
    gemm_options("gemm_sk_stages", stages)
    x = W.synth_normal(1, f"skx{Ci}{T}", (B, Ci, T))
    w = W.synth_normal(2, f"skw{Ci}{Co}", (Co, Ci, 1), std=1.0 / np.sqrt(Ci))
    b = W.synth_normal(3, "skb", (Co,), std=0.1)
    ref = O.conv1d(x, w, b)
    y = BV.conv1d(x, w, b, dtype=dtype)
    assert y.shape == ref.shape
    if dtype == "f32":
        np.testing.assert_allclose(y, ref, atol=3e-5, rtol=1e-5)
    else:
        assert rms(y - ref) / rms(ref) < tol
    assert np.array_equal(y, BV.conv1d(x, w, b, dtype=dtype))
    gemm_options("gemm_sk", 0)
    y0 = BV.conv1d(x, w, b, dtype=dtype)                    # one tile per workgroup: same products, other summation split
    if dtype == "f32":
        np.testing.assert_allclose(y, y0, atol=3e-5, rtol=1e-5)
    else:
        assert rms(y - y0) / rms(ref) < tol


@pytest.mark.parametrize("dtype,tol", [("f16", 6e-3), ("bf16", 4e-2)])
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("Ci,Co,T,B", [(1024, 1024, 1126, 2), (512, 3072, 700, 3), (64, 1280, 257, 1), (2048, 1024, 300, 1),
                                        (256, 1088, 1500, 1), (192, 2048, 4100, 1), (1024, 2048, 9000, 1), (512, 1280, 14000, 1)])
def test_eight_phase_256_tile_linear_vs_oracle(gemm_options, dtype, tol, order, Ci, Co, T, B):
    """gemm_ph8.hip: 256x256 tiles, two wave groups one barrier apart, half-tiles re-staged by counted LDS-DMA.  One K tile
    (the prologue alone), odd and even K tile counts, ragged M and N tails (out-of-range rows come back as zeros from the
    buffer range check), both tile orders, run-to-run identity, and agreement with the 128x128 kernels on the same data.
    The last two shapes have more tiles than the chip has CUs (288 and 275): their tail tiles are cut into K slices whose
    partial sums are added in slice order by the slice-0 workgroup (gemm_ph8_split_max = 1 switches that off)."""
    from mi355tts import _lib
    gemm_options("gemm_ph8", 1)
    gemm_options("gemm_ph8_min_tiles", 1)
    gemm_options("gemm_ph8_order", order)
    gemm_options("gemm_ph8_split_max", 4)
    gemm_options("gemm_ph8_split_min_nk", 1)
    x = W.synth_normal(1, f"p8x{Ci}{T}", (B, Ci, T))
    w = W.synth_normal(2, f"p8w{Ci}{Co}", (Co, Ci, 1), std=1.0 / np.sqrt(Ci))
    b = W.synth_normal(3, "p8b", (Co,), std=0.1)
    ref = O.conv1d(x, w, b)
    y = BV.conv1d(x, w, b, dtype=dtype)
    assert y.shape == ref.shape
    assert rms(y - ref) / rms(ref) < tol
    assert np.abs(y - ref).max() < 40 * tol * rms(ref)
    for _ in range(3):
        assert np.array_equal(y, BV.conv1d(x, w, b, dtype=dtype))
    gemm_options("gemm_ph8_split_max", 1)
    y1 = BV.conv1d(x, w, b, dtype=dtype)                    # tail tiles unsplit: same products, other summation split
    assert rms(y - y1) / rms(ref) < 1e-3 * tol + 1e-6
    gemm_options("gemm_ph8", 0)
    y0 = BV.conv1d(x, w, b, dtype=dtype)                    # 128x128 kernels: same products, same 64-deep fp32 accumulation order
    assert rms(y - y0) / rms(ref) < 1e-3 * tol + 1e-6


@pytest.mark.parametrize("Ci,Co,T,B", [(256, 1000, 1500, 1), (1024, 1024, 1126, 2), (128, 3072, 700, 2), (256, 2048, 2252, 1),
                                        (2048, 1024, 1126, 2)])
def test_f32_linear_as_exact_bf16_splits_vs_oracle(gemm_options, Ci, Co, T, B):
    """gemm_x3.hip (the round-2 kernel, now the fallback of gemm_x3p.hip): every fp32 product as six exact bf16 x bf16 partial
    products (three-way split of both operands, fp32 accumulation).  Same gate as the native fp32 MFMA path (atol 3e-5 against
    the oracle), agreement with the native kernel far inside that gate, an error against a float64 evaluation no larger than
    the native kernel's, ragged M / N tails, tiles split between workgroups, run-to-run identity."""
    gemm_options("gemm_f32_x3", 1)
    gemm_options("gemm_f32_x3p", 0)                        # the round-2 kernel itself (panel-plane form: next test)
    x = W.synth_normal(1, f"x3x{Ci}{T}", (B, Ci, T))
    w = W.synth_normal(2, f"x3w{Ci}{Co}", (Co, Ci, 1), std=1.0 / np.sqrt(Ci))
    b = W.synth_normal(3, "x3b", (Co,), std=0.1)
    ref = O.conv1d(x, w, b)
    y = BV.conv1d(x, w, b, dtype="f32")
    np.testing.assert_allclose(y, ref, atol=3e-5, rtol=1e-5)
    assert np.array_equal(y, BV.conv1d(x, w, b, dtype="f32"))
    gemm_options("gemm_f32_x3", 0)
    y0 = BV.conv1d(x, w, b, dtype="f32")                    # v_mfma_f32_32x32x2_f32
    np.testing.assert_allclose(y0, ref, atol=3e-5, rtol=1e-5)
    assert np.abs(y - y0).max() < 1e-5
    # the split loses nothing against native fp32: both sit at the same distance from a float64 evaluation
    ref64 = np.einsum("oc,bct->bot", w[:, :, 0].astype(np.float64), x.astype(np.float64)) + b.astype(np.float64)[None, :, None]
    e_x3, e_native = rms(y - ref64), rms(y0 - ref64)
    assert e_x3 < 1.5 * e_native + 1e-9, (e_x3, e_native)


@pytest.mark.parametrize("planes", [2, 3])
@pytest.mark.parametrize("grid", [0, 1, 2, 4, 8])
@pytest.mark.parametrize("noalign", [0, 1])
@pytest.mark.parametrize("Ci,Co,T,B", [(1024, 1024, 1126, 2), (1024, 3072, 1126, 2), (2048, 1024, 1126, 2), (1024, 2048, 2252, 1),
                                        (256, 1024, 1500, 1), (1024, 1024, 1126, 6), (64, 1280, 700, 2)])
def test_f32_linear_panel_planes_vs_oracle(gemm_options, planes, grid, noalign, Ci, Co, T, B):
    """gemm_x3p.hip (round 3): BOTH operands pre-split into panel planes — three bf16 planes (six exact partial products)
    or two fp16 planes {hi, lo * 2^11} (three partial products on two accumulator sets) — eight waves as two k16 groups,
    2-D XCD bands (gemm_x3p_grid = GR, 0 = automatic) and the cyclic K walk (gemm_x3p_noalign = 1 switches it off).  Same
    gates as the round-2 kernel: atol 3e-5 against the oracle, < 1e-5 from the native fp32 MFMA, error against float64 no
    larger than native, run-to-run identity; the DiT shapes at one utterance (M = 2252) and three (M = 6756: several tiles
    per workgroup), K = 64 ... 2048, a ragged last row panel."""
    gemm_options("gemm_f32_planes", planes)
    gemm_options("gemm_f32_x3", 1)
    gemm_options("gemm_f32_x3p", 1)
    gemm_options("gemm_x3p_grid", grid)
    gemm_options("gemm_x3p_noalign", noalign)
    x = W.synth_normal(1, f"x3x{Ci}{T}", (B, Ci, T))
    w = W.synth_normal(2, f"x3w{Ci}{Co}", (Co, Ci, 1), std=1.0 / np.sqrt(Ci))
    b = W.synth_normal(3, "x3b", (Co,), std=0.1)
    ref = O.conv1d(x, w, b)
    y = BV.conv1d(x, w, b, dtype="f32")
    np.testing.assert_allclose(y, ref, atol=3e-5, rtol=1e-5)
    assert np.array_equal(y, BV.conv1d(x, w, b, dtype="f32"))
    gemm_options("gemm_f32_x3p", 0)
    y2 = BV.conv1d(x, w, b, dtype="f32")                    # round-2 kernel: same arithmetic, other summation order
    assert np.abs(y - y2).max() < 1e-5 and not np.array_equal(y, y2)
    gemm_options("gemm_f32_x3", 0)
    y0 = BV.conv1d(x, w, b, dtype="f32")                    # v_mfma_f32_32x32x2_f32
    assert np.abs(y - y0).max() < 1e-5
    ref64 = np.einsum("oc,bct->bot", w[:, :, 0].astype(np.float64), x.astype(np.float64)) + b.astype(np.float64)[None, :, None]
    e_x3, e_native = rms(y - ref64), rms(y0 - ref64)
    assert e_x3 < 1.5 * e_native + 1e-9, (e_x3, e_native)


@pytest.mark.parametrize("scale", [1e-6, 1e-3, 1.0, 300.0, 3e4])
def test_f32_linear_fp16_pairs_over_the_operand_range(gemm_options, scale):
    """The two-plane form stores an operand as fp16(a) and fp16((a - hi) * 2^11): 22 significant bits with the residual
    kept in the exponent range of the value, |a| clamped at 65504.  Its error is relative (2^-23) down to |a| ~ 2^-12 and
    ABSOLUTE (2^-36 = 1.5e-11 per operand) below that, where fp16(a) itself goes subnormal.  Operands from 1e-3 to 3e4 in
    magnitude: the relative error against float64 stays at the native fp32 MFMA's (and the three-plane form's); a tensor
    that is 1e-6 throughout: inside the absolute floor."""
    Ci, Co, T, B = 1024, 1024, 1126, 2
    x = (W.synth_normal(1, f"rx{Ci}{T}", (B, Ci, T)) * scale).astype(np.float32)
    x = np.clip(x, -65000.0, 65000.0)
    w = W.synth_normal(2, f"rw{Ci}{Co}", (Co, Ci, 1), std=1.0 / np.sqrt(Ci))
    ref64 = np.einsum("oc,bct->bot", w[:, :, 0].astype(np.float64), x.astype(np.float64))
    err = {}
    for name, opts in (("pairs", {"gemm_f32_planes": 2}), ("bf16x3", {"gemm_f32_planes": 3}), ("native", {"gemm_f32_x3": 0})):
        gemm_options("gemm_f32_x3", 1); gemm_options("gemm_f32_x3p", 1)
        for k, v in opts.items():
            gemm_options(k, v)
        err[name] = rms(BV.conv1d(x, w, None, dtype="f32") - ref64)
    rel = {k: v / rms(ref64) for k, v in err.items()}
    print(f"scale {scale:g}: relative rms error against float64: {rel}")
    if scale >= 1e-3:
        assert rel["pairs"] < 1.5 * rel["native"] and rel["pairs"] < 1.5 * rel["bf16x3"] and rel["pairs"] < 1e-6, rel
    else:       # sum over K of w * (2^-36 operand error): sqrt(K) * rms(w) = 1 here
        assert err["pairs"] < 4 * 2.0 ** -36, err


@pytest.mark.parametrize("C,groups,k,T,B", [(1024, 16, 31, 1126, 2), (512, 8, 31, 300, 1), (256, 4, 9, 515, 3)])
def test_f32_grouped_conv_fp16_pairs_in_registers(gemm_options, C, groups, k, T, B):
    """The DiT's position convolution (Conv1d k = 31, 16 groups of 64 channels) in fp32: conv_gemm_dma_kernel splits both
    operands into fp16 {hi, lo} pairs in registers (three 16-bit MFMAs per k-step on two accumulator sets instead of eight
    fp32 MFMAs; option gemm_f32_n64_pairs).  Against the oracle, against the native fp32 MFMA form of the same kernel, and
    against float64: no further from it than native."""
    x = W.synth_normal(41, f"gx{C}{T}", (B, C, T))
    w = W.synth_normal(42, f"gw{C}{k}", (C, C // groups, k), std=1.0 / np.sqrt(C // groups * k))
    b = W.synth_normal(43, "gb", (C,), std=0.1)
    cgo = C // groups
    ref = np.concatenate([O.conv1d(x[:, gi * cgo:(gi + 1) * cgo], w[gi * cgo:(gi + 1) * cgo], b[gi * cgo:(gi + 1) * cgo], padding=k // 2)
                          for gi in range(groups)], axis=1)
    gemm_options("gemm_f32_n64_pairs", 1)
    y = BV.conv1d(x, w, b, padding=k // 2, groups=groups, dtype="f32")
    assert np.array_equal(y, BV.conv1d(x, w, b, padding=k // 2, groups=groups, dtype="f32"))
    gemm_options("gemm_f32_n64_pairs", 0)
    y0 = BV.conv1d(x, w, b, padding=k // 2, groups=groups, dtype="f32")
    np.testing.assert_allclose(y, ref, atol=3e-5, rtol=1e-5)
    assert np.abs(y - y0).max() < 3e-5 and not np.array_equal(y, y0)        # K = 1984: two fp32 summation orders
    xp = np.pad(x.astype(np.float64), ((0, 0), (0, 0), (k // 2, k // 2)))
    cg = C // groups
    ref64 = np.zeros((B, C, T))
    for gi in range(groups):
        win = np.lib.stride_tricks.sliding_window_view(xp[:, gi * cg:(gi + 1) * cg], k, axis=2)       # (B, cg, T, k)
        ref64[:, gi * cg:(gi + 1) * cg] = np.einsum("bctk,ock->bot", win, w[gi * cg:(gi + 1) * cg].astype(np.float64))
    ref64 += b.astype(np.float64)[None, :, None]
    e_pairs, e_native = rms(y - ref64), rms(y0 - ref64)
    print(f"grouped conv C={C} k={k}: rms error against float64: pairs {e_pairs:.3e}, native fp32 MFMA {e_native:.3e}")
    assert e_pairs < 1.5 * e_native + 1e-9, (e_pairs, e_native)


@pytest.mark.parametrize("f32_dma,small,buf", [(1, 1, 1), (1, 0, 1), (1, 1, 0), (1, 0, 0), (0, 1, 1)])
def test_f32_gemm_dma_and_register_staged_agree_with_oracle(gemm_options, f32_dma, small, buf):
    # fp32 linears / convs with N > 64 run on the LDS-DMA kernel (32-float chunks, k pairs (e, e+4) per MFMA): 64x64 tiles
    # when there are few 128x128 tiles (gemm_f32_small), buffer-descriptor or flat-address DMA (gemm_buf);
    # gemm_f32_dma = 0 keeps the register-staged kernel covered
    gemm_options("gemm_f32_dma", f32_dma)
    gemm_options("gemm_f32_small", small)
    gemm_options("gemm_buf", buf)
    for Ci, Co, k, d, T, B in [(384, 384, 7, 3, 300, 2), (100, 200, 3, 1, 129, 1), (1024, 3072, 1, 1, 140, 1)]:
        x = W.synth_normal(31, f"fx{Ci}{k}", (B, Ci, T))
        w = W.synth_normal(32, f"fw{Ci}{Co}{k}", (Co, Ci, k), std=1.0 / np.sqrt(Ci * k))
        b = W.synth_normal(33, "fb", (Co,), std=0.1)
        pad = (k * d - d) // 2
        ref = O.conv1d(x, w, b, dilation=d, padding=pad)
        y = BV.conv1d(x, w, b, dilation=d, padding=pad)
        np.testing.assert_allclose(y, ref, atol=2e-5, rtol=1e-5)


# ---------------------------------------------------------------------------------------------
# IndexTTS graph F (config 5 vocoder): pre-LayerNorm, speaker-conditioning biases, k = u ConvTranspose, biased conv_post
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ci,Co,u,k,T", [(96, 48, 4, 4, 50), (48, 24, 2, 4, 33), (16, 8, 4, 8, 5)])
def test_conv_transpose_kernel_equals_stride(Ci, Co, u, k, T):
    x = W.synth_normal(1, f"xtk{Ci}", (1, Ci, T))
    w = W.synth_normal(2, f"wtk{Ci}", (Ci, Co, k), std=1.0 / np.sqrt(Ci))
    b = W.synth_normal(3, "btk", (Co,), std=0.1)
    ref = O.conv_transpose1d(x, w, b, stride=u, padding=(k - u) // 2)
    y = BV.conv_transpose1d(x, w, b, stride=u, padding=(k - u) // 2)
    assert y.shape == ref.shape == (1, Co, T * u)
    np.testing.assert_allclose(y, ref, atol=2e-5, rtol=1e-5)


def test_indextts_graph_f_golden_and_oracle(golden_dir):
    g = np.load(os.path.join(golden_dir, "indextts_f.npz"))
    cfg = BigVGANConfig.indextts()
    st = W.synth_state(W.bigvgan_spec(cfg), 9527)
    conds = [g[f"cond{i}"] for i in range(cfg.num_upsamples)] + [g["cond_pre"]]
    v = BV.BigVGANVocoder(cfg, st, dtype="f32")
    w, wf = v.run_latent(g["latent"], conds, return_float=True)
    assert w.shape == g["wav_i16"].shape and w.dtype == np.int16
    assert np.abs(w.astype(np.int32) - g["wav_i16"].astype(np.int32)).max() <= 3        # vs the reference wrapper
    ref = O.indextts_f_float(cfg, st, g["latent"], [c.reshape(-1) for c in conds])
    assert rms(wf - ref) < 1e-5                                                          # vs the oracle, fp32
    with pytest.raises(Exception):
        v.run(np.zeros((1, cfg.num_mels, 4), np.float32))                                # wrong entry point for this handle
    with pytest.raises(ValueError):
        v.run_latent(g["latent"][:2], conds)                                             # fewer than 3 latent rows
    v.close()
    v16 = BV.BigVGANVocoder(cfg, st, dtype="f16")
    w16 = v16.run_latent(g["latent"], conds)
    assert rms((w16.astype(np.float64) - g["wav_i16"]) / 32767.0) < 2e-2
    v16.close()
