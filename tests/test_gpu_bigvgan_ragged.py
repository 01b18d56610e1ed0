"""GPU: ragged BigVGAN batches — items of different lengths in one forward (padded slabs of Fmax = max F_b frames, a device
frame table, length-aware kernels; include/mi355tts.h mi_bigvgan_forward_ragged / mi_bigvgan_forward_latent_ragged /
mi_f5_synthesize_mel_ragged).

  * equal lengths through the ragged entry == the uniform entry, bit for bit, with the " + lengths" kernels engaged;
  * every item against the numpy oracle at its own length (full architecture; lengths on a 256-row tile edge), and against
    itself run alone;
  * isolation (other items' mels and lengths at the same (B, Fmax)), stale workspace, the three stream modes;
  * full size against the reference fixture; graph F (IndexTTS) against its golden and oracle;
  * F5 -> BigVGAN: the ragged mels equal the uniform ones and the device chain equals the host chain;
  * argument errors leave both handles usable.
"""
import os

import numpy as np
import pytest

from mi355tts import _lib
from mi355tts import weights as W
from mi355tts import bigvgan as BV
from mi355tts.config import BigVGANConfig, F5Config
from mi355tts.f5 import F5Engine
from oracle import bigvgan_np as O

pytestmark = pytest.mark.gpu

MI_OK, MI_EINVAL = 0, -1                 # include/mi355tts.h
MIX = (12, 5, 9, 1, 65, 64)          # 65 / 64 frames: stage 0 (x8) runs 520 / 512 rows, one row past / on a 256-row tile edge


def rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, np.float64)))))


def _mel(F, seed):
    return W.synth_normal(seed, "mel", (1, 100, F), std=2.0, mean=-2.0).clip(-11.5, 2.5)[0]


def _close_lsb(a, b):
    """test_gpu_f5_ragged._close_lsb: int16 waveforms within 2 LSB, fewer than 1 % of the samples off at all."""
    d = np.abs(a.astype(np.int32) - b.astype(np.int32))
    return a.shape == b.shape and d.max(initial=0) <= 2 and (d > 0).mean() < 0.01


@pytest.fixture(scope="module")
def full_state():
    cfg = BigVGANConfig()
    return cfg, W.synth_state(W.bigvgan_spec(cfg), 9527)


@pytest.fixture(scope="module")
def vocs(full_state):
    cfg, st = full_state
    vs = {dt: BV.BigVGANVocoder(cfg, st, dtype=dt) for dt in ("f32", "f16", "bf16")}
    yield vs
    for v in vs.values():
        v.close()


def _ragged_profiled(v, mels):
    _lib.prof_reset(); _lib.prof_enable(("conv_gemm", "aa_act", "conv_post", "other"))
    try:
        w = v.run_ragged(mels)
    finally:
        _lib.prof_enable(())
    return w, {k["kernel"] for k in _lib.prof_kernels() if k["launches"] > 0}


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_equal_lengths_match_uniform_bitwise(vocs, dtype):
    v = vocs[dtype]
    mel = np.stack([_mel(40, 5 + b) for b in range(3)])
    ref = v.run(mel)
    w, kernels = _ragged_profiled(v, list(mel))
    for b in range(3):
        assert np.array_equal(w[b], ref[b:b + 1]), b
    lk = {k for k in kernels if k.endswith(" + lengths")}
    assert any(k.startswith("conv_gemm") for k in lk) and any(k.startswith("aa_") for k in lk), sorted(kernels)
    assert any(k.startswith("conv_post_kernel") for k in lk) and any(k.startswith("ncl_to_nlc_kernel") for k in lk), sorted(kernels)
    assert not kernels - lk, sorted(kernels - lk)                     # every launch of the forward is a length-aware one


def test_each_item_matches_oracle_full_arch(full_state, vocs):
    """Gates of test_generator_full_arch_*: fp32 RMS < 1e-5 and int16 <= 2 LSB against bigvgan_int16; f16 < 2e-2."""
    cfg, st = full_state
    mels = [_mel(F, 30 + b) for b, F in enumerate(MIX)]
    w32, f32 = vocs["f32"].run_ragged(mels, return_float=True)
    _, f16 = vocs["f16"].run_ragged(mels, return_float=True)
    for b, (m, F) in enumerate(zip(mels, MIX)):
        ref = O.generator(cfg, st, m[None])
        assert f32[b].shape == ref.shape == (1, 1, F * 256 + 30)
        assert rms(f32[b] - ref) < 1e-5, (b, rms(f32[b] - ref))
        wr = O.bigvgan_int16(cfg, st, m[None])
        assert np.abs(w32[b].astype(np.int32) - wr.astype(np.int32)).max() <= 2, b
        assert rms(f16[b] - ref) < 2e-2, (b, rms(f16[b] - ref))
        assert rms(ref) > 1e-3


def test_each_item_matches_itself_alone(full_state, vocs):
    """fp32: within 2 LSB of the item alone (_close_lsb); f16: the oracle gate of item 2.  bf16 has no oracle gate in the suite; the
    issue's gate is 3x the measured difference to the item alone, and that difference measured 0 on an MI355X (the 16-bit conv
    kernels of both tile plans accumulate every output in the same (channel chunk, tap) order), so bf16 must be bit-identical."""
    cfg, st = full_state
    mels = [_mel(F, 30 + b) for b, F in enumerate(MIX)]
    w32 = vocs["f32"].run_ragged(mels)
    _, f16 = vocs["f16"].run_ragged(mels, return_float=True)
    _, b16 = vocs["bf16"].run_ragged(mels, return_float=True)
    for b, m in enumerate(mels):
        assert _close_lsb(w32[b], vocs["f32"].run(m[None])), b
        ref = O.generator(cfg, st, m[None])
        assert rms(f16[b] - ref) < 2e-2, b
        alone = vocs["bf16"].run_float(m[None])
        assert np.array_equal(b16[b], alone), (b, rms(b16[b] - alone))


def _profiled(fn):
    _lib.prof_reset(); _lib.prof_enable(("conv_gemm",))
    try:
        out = fn()
    finally:
        _lib.prof_enable(())
    return out, {k["kernel"] for k in _lib.prof_kernels() if k["launches"] > 0}


def test_past_the_big_tile_switch_f16(full_state, vocs):
    """B = 8 at Fmax = 520: the uniform plan puts the stage-0 AMP convolutions (N = 768, K >= 2304) on the 256x256 tile.  That tile
    has no lengths instantiation; the ragged launches take the 256x192 one instead.  Every item equals itself alone, bit for bit,
    and the short ones meet the f16 oracle gate."""
    cfg, st = full_state
    v = vocs["f16"]
    frames = (520, 12, 5, 300, 97, 1, 64, 410)
    mels = [_mel(F, 120 + b) for b, F in enumerate(frames)]
    big = "conv_gemm_dma3_kernel<_Float16, _Float16, 256, 256, 128, 64, 2, true>"
    _, uni = _profiled(lambda: v.run(np.stack([_mel(520, 130 + b) for b in range(8)])))
    assert big in uni, sorted(uni)                                   # the test sits past the switch
    (wav, fl), rag = _profiled(lambda: v.run_ragged(mels, return_float=True))
    assert not any(k.startswith("conv_gemm_dma3_kernel<_Float16, _Float16, 256, 256") for k in rag), sorted(rag)
    assert "conv_gemm_dma3_kernel<_Float16, _Float16, 256, 192, 64, 96, 2, true> + lengths" in rag, sorted(rag)
    for b, m in enumerate(mels):
        alone = v.run_float(m[None])
        assert np.array_equal(fl[b], alone), (b, rms(fl[b] - alone))
        assert np.array_equal(wav[b], v.run(m[None])), b
        if frames[b] <= 12:
            assert rms(fl[b] - O.generator(cfg, st, m[None])) < 2e-2, b


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_isolation(vocs, dtype):
    """Other items' mels and lengths change, B and Fmax stay: item 1 stays bit-identical."""
    v = vocs[dtype]
    keep = _mel(33, 77)
    a = v.run_ragged([_mel(70, 1), keep, _mel(9, 2)])
    b = v.run_ragged([_mel(21, 3), keep, _mel(70, 4)])
    assert np.array_equal(a[1], b[1])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_stale_workspace(full_state, vocs, dtype):
    """A larger uniform call first on the same handle: the ragged result equals a fresh handle's, bit for bit, and is finite."""
    cfg, st = full_state
    mels = [_mel(F, 50 + b) for b, F in enumerate((40, 7, 23))]
    v = vocs[dtype]
    v.run(np.stack([_mel(40, 90 + b) for b in range(3)]) + 3.0)
    _, dirty = v.run_ragged(mels, return_float=True)
    fresh = BV.BigVGANVocoder(cfg, st, dtype=dtype)
    try:
        _, clean = fresh.run_ragged(mels, return_float=True)
    finally:
        fresh.close()
    for x, y in zip(dirty, clean):
        assert np.all(np.isfinite(x)) and np.array_equal(x, y)


def test_stream_modes_bit_identical(vocs):
    mels = [_mel(F, 60 + b) for b, F in enumerate((24, 11, 3))]
    v = vocs["f16"]
    saved = _lib.get_option("bigvgan_streams")
    try:
        _lib.set_option("bigvgan_streams", 1)
        ref = v.run_ragged(mels)
        for ns in (2, 3):
            _lib.set_option("bigvgan_streams", ns)
            out = v.run_ragged(mels)
            assert all(np.array_equal(a, b) for a, b in zip(out, ref)), ns
    finally:
        _lib.set_option("bigvgan_streams", saved)


def test_full_size_reference_fixture(full_state, vocs, golden_dir):
    """test_full_size_reference_fixture's gates for the fixture mel as item 0 of a ragged batch."""
    cfg, _ = full_state
    gf = np.load(os.path.join(golden_dir, "bigvgan_full.npz"))
    ref = gf["wav_i16"].astype(np.float64)
    mel8 = W.bigvgan_synthetic_mel(cfg, 8, 512, 0)
    w = vocs["f32"].run_ragged([mel8[0], mel8[1][:, :300], mel8[2][:, :97], mel8[3][:, :1]])
    assert [x.shape[-1] for x in w] == [512 * 256 + 30, 300 * 256 + 30, 97 * 256 + 30, 286]
    d = np.abs(w[0][0, 0].astype(np.int32) - gf["wav_i16"].astype(np.int32))
    err32 = rms((w[0][0, 0] - ref) / 32767.0)
    assert err32 < 1e-4, err32
    assert d.max() <= 4 and (d > 1).mean() < 1e-3, (d.max(), (d > 1).mean())
    frames = [512, 470, 390, 300, 512, 200, 150, 512]
    mels = [mel8[b][:, :f] for b, f in enumerate(frames)]
    mels[4] = mels[7] = mel8[0]                                        # the fixture mel at three slab positions
    w16 = vocs["f16"].run_ragged(mels)
    err16 = rms((w16[0][0, 0] - ref) / 32767.0)
    assert err16 < 4e-3, err16
    assert np.array_equal(w16[0], w16[4]) and np.array_equal(w16[0], w16[7])
    print(f"ragged full size vs reference: fp32 rms {err32:.2e} (max |d| {d.max()} LSB), fp16 rms {err16:.2e}")


def test_graph_f_ragged(golden_dir):
    g = np.load(os.path.join(golden_dir, "indextts_f.npz"))
    cfg = BigVGANConfig.indextts()
    st = W.synth_state(W.bigvgan_spec(cfg), 9527)
    conds = [g[f"cond{i}"] for i in range(cfg.num_upsamples)] + [g["cond_pre"]]
    lat = g["latent"]
    T = lat.shape[0]
    items = [lat[:3], lat, lat[:17], lat[: max(3, T // 2)]]
    v = BV.BigVGANVocoder(cfg, st, dtype="f32")
    try:
        w, wf = v.run_latent_ragged(items, conds, return_float=True)
        assert w[1].shape == g["wav_i16"].shape
        assert np.abs(w[1].astype(np.int32) - g["wav_i16"].astype(np.int32)).max() <= 3
        for b, x in enumerate(items):
            ref = O.indextts_f_float(cfg, st, x, [c.reshape(-1) for c in conds])
            assert wf[b].shape == ref.shape and rms(wf[b] - ref) < 1e-5, (b, rms(wf[b] - ref))
        with pytest.raises(ValueError):
            v.run_latent_ragged([lat, lat[:2]], conds)
        L = _lib.load()
        flat = v._flat_conds(conds)
        x = np.ascontiguousarray(np.concatenate([lat, lat[:2]]), np.float32)
        tc = np.asarray([T, 2], np.int64)
        out = np.zeros(10 * T * cfg.hop, np.int16)
        lens = np.zeros(2, np.int64)
        assert L.mi_bigvgan_forward_latent_ragged(v._h, 2, x.ctypes.data, tc.ctypes.data, flat.ctypes.data, flat.size, out.ctypes.data,
                                                  None, out.size, lens.ctypes.data, _lib.MI_HOST) == MI_EINVAL
        assert np.array_equal(v.run_latent_ragged([lat], conds)[0], w[1])                      # the handle is still usable
    finally:
        v.close()


F5_REQS = [(4096, 20, 60), (6144, 12, 45), (3000, 30, 70)]     # (prompt samples, text ids, max_duration)


def _f5_request(cfg, u, L, T):
    t = np.arange(L) / cfg.sample_rate
    a = 0.1 * 32767 * np.sin(2 * np.pi * (180 + 40 * u) * t) + W.synth_normal(50 + u, "audio", (L,), std=500.0)
    ids = (np.arange(T) * (7 + u)) % (cfg.text_num_embeds - 1)
    return np.clip(np.round(a), -32768, 32767).astype(np.int16), ids.astype(np.int32)


@pytest.fixture(scope="module")
def f5_small():
    cfg = F5Config.small()
    eng = F5Engine(cfg, W.synth_state(W.f5_spec(cfg), 9527), dtype="f32")
    vcfg = BigVGANConfig(num_mels=100, upsample_initial_channel=64, upsample_rates=(4, 2), upsample_kernel_sizes=(8, 4))
    voc = BV.BigVGANVocoder(vcfg, W.synth_state(W.bigvgan_spec(vcfg), 9527), dtype="f32")
    yield cfg, eng, voc
    eng.close()
    voc.close()


def test_f5_mel_ragged_to_bigvgan(f5_small):
    import torch
    cfg, eng, voc = f5_small
    reqs = [_f5_request(cfg, u, L, T) for u, (L, T, _) in enumerate(F5_REQS)]
    audios, ids = [r[0] for r in reqs], [r[1] for r in reqs]
    N = [n for _, _, n in F5_REQS]
    noise = [W.synth_normal(70 + u, "noise", (n, cfg.mel_dim)) for u, n in enumerate(N)]
    # equal lengths: == the uniform entry, bit for bit
    n2 = [noise[0], W.synth_normal(79, "noise", (N[0], cfg.mel_dim))]
    eq = eng.synthesize_mel_ragged([audios[0]] * 2, [ids[0]] * 2, [N[0]] * 2, noise=n2)
    uni = eng.synthesize_mel(np.stack([audios[0]] * 2), np.stack([ids[0]] * 2), N[0], noise=np.stack(n2))
    for u in range(2):
        assert np.array_equal(eq[u], uni[u]), u
    # every utterance == itself alone (fp32, rel RMS <= 1e-5)
    mels = eng.synthesize_mel_ragged(audios, ids, N, noise=noise)
    for u in range(3):
        alone = eng.synthesize_mel(audios[u][None], ids[u][None], N[u], noise=noise[u][None])[0]
        assert mels[u].shape == alone.shape == (cfg.mel_dim, N[u] - cfg.ref_frames(audios[u].size))
        assert rms(mels[u] - alone) <= 1e-5 * rms(alone), u
    host = voc.run_ragged(mels)
    # the device chain: no host round trip between the two engines
    dev = torch.device("cuda", 0)
    a_cat = torch.from_numpy(np.concatenate(audios)).to(dev)
    t_cat = torch.from_numpy(np.concatenate(ids)).to(dev)
    n_cat = torch.from_numpy(np.concatenate(noise).astype(np.float32)).to(dev)
    mel_cat, frames = eng.synthesize_mel_ragged_torch(a_cat, [a.size for a in audios], t_cat, [t.size for t in ids], N, noise=n_cat)
    assert frames == [m.shape[1] for m in mels]
    assert np.array_equal(mel_cat.cpu().numpy(), np.concatenate([m.reshape(-1) for m in mels]))
    wav_cat, lens = voc.run_ragged_torch(mel_cat, frames)
    assert lens == [x.shape[-1] for x in host]
    assert np.array_equal(wav_cat.cpu().numpy(), np.concatenate([x.reshape(-1) for x in host]))


def test_argument_errors_leave_handles_usable(vocs, f5_small):
    v = vocs["f32"]
    L = _lib.load()
    mels = [_mel(10, 1), _mel(4, 2)]
    ref = v.run_ragged(mels)
    x = np.ascontiguousarray(np.concatenate([m.reshape(-1) for m in mels]), np.float32)
    out = np.zeros(20 * 256, np.int16)
    lens = np.zeros(2, np.int64)

    def call(B, frames, cap):
        fr = np.asarray(frames, np.int64)
        return L.mi_bigvgan_forward_ragged(v._h, B, x.ctypes.data, fr.ctypes.data, out.ctypes.data, None, cap, lens.ctypes.data,
                                           _lib.MI_HOST)
    assert call(0, [10, 4], out.size) == MI_EINVAL                         # B < 1
    assert call(2, [10, 0], out.size) == MI_EINVAL                         # F_b < 1
    assert call(2, [10, 1 << 22], out.size) == MI_EINVAL                   # past the uniform path's frame limit
    assert call(2, [10, 4], 14 * 256 + 59) == MI_EINVAL                    # out_cap one below the sum
    with pytest.raises(ValueError):
        v.run_ragged([_mel(10, 1), np.zeros((80, 4), np.float32)])
    gcfg = BigVGANConfig.indextts()
    g = BV.BigVGANVocoder(gcfg, W.synth_state(W.bigvgan_spec(gcfg), 9527), dtype="f32")
    try:
        fr = np.asarray([10, 4], np.int64)
        assert L.mi_bigvgan_forward_ragged(g._h, 2, x.ctypes.data, fr.ctypes.data, out.ctypes.data, None, out.size, lens.ctypes.data,
                                           _lib.MI_HOST) == MI_EINVAL     # a graph-F handle
    finally:
        g.close()
    assert call(2, [10, 4], 14 * 256 + 60) == MI_OK
    assert all(np.array_equal(a, b) for a, b in zip(v.run_ragged(mels), ref))
    cfg, eng, _ = f5_small
    a, t = _f5_request(cfg, 0, 4096, 20)
    with pytest.raises(ValueError):
        eng.synthesize_mel_ragged([a], [t], [cfg.ref_frames(a.size)])              # no generated frame
    al, tl, nl = (np.asarray([v_], np.int64) for v_ in (a.size, t.size, 60))
    mel = np.zeros(10, np.float32)
    nf = np.zeros(1, np.int64)
    assert L.mi_f5_synthesize_mel_ragged(eng._h, 1, a.ctypes.data, al.ctypes.data, t.ctypes.data, tl.ctypes.data, nl.ctypes.data,
                                         None, 9527, mel.ctypes.data, mel.size, nf.ctypes.data, _lib.MI_HOST) == MI_EINVAL
    assert eng.synthesize_mel_ragged([a], [t], [60])[0].shape == (cfg.mel_dim, 60 - cfg.ref_frames(a.size))
