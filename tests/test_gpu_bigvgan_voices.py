"""GPU: several voices in one ragged graph-F forward (include/mi355tts.h mi_bigvgan_forward_latent_voices;
BigVGANVocoder.run_latent_voices / run_latent_voices_torch).  A kernel builds the (B, total_cond) table of layer bias + speaker
conditioning on the device and conv_pre and the six upsamplers read their bias row by batch item (ConvGemm::bias_bstride).

  1. every item against the numpy oracle with ITS voice (fp32 1e-5, the golden latent within 3 LSB of the reference wrapper's
     int16, f16 2e-2: the gates of test_indextts_graph_f_golden_and_oracle / test_graph_f_ragged), and far from the oracle with
     another voice;
  2. isolation, bit for bit: item b of a mixed batch == item b of the one-voice batch with voice_of[b] for everyone;
  3. every length-aware GEMM instantiation the planner can give the seven layers carries the table (profiler names end in
     " + lengths + item bias"), including a batch past the big-tile switch;
  4. the device-resident form; no table cached between calls; no stale rows after a larger batch;
  5. argument errors are MI_EINVAL / ValueError and leave the handle usable.
"""
import os

import numpy as np
import pytest

from mi355tts import _lib
from mi355tts import weights as W
from mi355tts import bigvgan as BV
from mi355tts.config import BigVGANConfig
from oracle import bigvgan_np as O

pytestmark = pytest.mark.gpu

MI_OK, MI_EINVAL = 0, -1                   # include/mi355tts.h
F1 = (12, 5, 9, 1, 3, 7)                   # test 1: frames per item (T_codes = F + 2); item 4 is the golden latent
VO = (2, 0, 1, 0, 2, 1)                    # unsorted on purpose
MIX = (12, 5, 9, 1, 65, 64)                # test 2: 65 / 64 frames put stage 0 (x4) one row past / on a tile edge, as in the ragged suite
BIG = (520, 12, 5, 300, 97, 1, 64, 410)    # test 3: f16, past the big-tile switch (test_past_the_big_tile_switch_f16's frames)
BIG_VO = (3, 2, 0, 1, 3, 0, 1, 2)          # items 1, 2, 5 (F = 12, 5, 1) are items 0, 1, 3 of test 1 with the same voices
ITEM_BIAS = " + lengths + item bias"


def rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, np.float64)))))


def _lat(F, seed):
    return W.synth_normal(seed, "lat", (F + 2, 1280), std=1.0)


@pytest.fixture(scope="module")
def env(golden_dir):
    cfg = BigVGANConfig.indextts()
    st = W.synth_state(W.bigvgan_spec(cfg), 9527)
    g = np.load(os.path.join(golden_dir, "indextts_f.npz"))
    sizes = [cfg.stage_channels(i) for i in range(cfg.num_upsamples)] + [cfg.upsample_initial_channel]
    voices = [[g[f"cond{i}"].reshape(-1) for i in range(cfg.num_upsamples)] + [g["cond_pre"].reshape(-1)]]
    for v in range(1, 4):                   # 0.2: the spread of the fixture's own seven vectors (std 0.196 - 0.247)
        voices.append([W.synth_normal(100 * v + i, "cond", (n,), std=0.2) for i, n in enumerate(sizes)])
    lat1 = [_lat(F, 300 + b) for b, F in enumerate(F1)]
    lat1[4] = np.ascontiguousarray(g["latent"], np.float32)
    assert lat1[4].shape[0] == F1[4] + 2
    vocs = {}
    oracle = {}

    def voc(dtype):
        if dtype not in vocs:
            vocs[dtype] = BV.BigVGANVocoder(cfg, st, dtype=dtype)
        return vocs[dtype]

    def ref(b, v):
        """float oracle of item b of test 1 spoken by voice v: computed once, shared, never written to"""
        if (b, v) not in oracle:
            r = O.indextts_f_float(cfg, st, lat1[b], voices[v])
            r.setflags(write=False)
            oracle[(b, v)] = r
        return oracle[(b, v)]

    class E:
        pass
    e = E()
    e.cfg, e.st, e.g, e.voices, e.lat1, e.voc, e.ref = cfg, st, g, voices, lat1, voc, ref
    yield e
    for v in vocs.values():
        v.close()


def _ref_i16(ref_float):
    """O.indextts_f_int16 is O.indextts_f_float followed by this line (oracle/bigvgan_np.py; tests/test_bigvgan_voices_layout.py
    holds the two to each other on the golden latent), so the float oracle computed for the fp32 gate serves the f16 gate too."""
    return (np.clip(ref_float, -1.0, 1.0) * np.float32(32767.0)).astype(np.int16)


@pytest.fixture(scope="module")
def run1(env):
    """test 1's forwards, once: fp32 (int16 + float) and f16 (int16) with voice_of = VO, and fp32 with item 4 on voice 0"""
    w32, f32 = env.voc("f32").run_latent_voices(env.lat1, env.voices[:3], VO, return_float=True)
    vo_g = list(VO)
    vo_g[4] = 0
    w32g, f32g = env.voc("f32").run_latent_voices(env.lat1, env.voices[:3], vo_g, return_float=True)
    w16 = env.voc("f16").run_latent_voices(env.lat1, env.voices[:3], VO)
    return w32, f32, w32g, f32g, w16


# ---- 1. each item against the oracle with its own voice ---------------------------------------------------------------------------
@pytest.mark.parametrize("b", range(len(F1)))
def test_each_item_matches_the_oracle_with_its_voice(env, run1, b):
    """fp32: rms(float - oracle(item, its voice)) < 1e-5; the float output is > 1e-2 rms away from the oracle with another voice (so
    a layer that read another item's row could not pass); f16: rms(int16 difference / 32767) < 2e-2 against the int16 oracle."""
    w32, f32, _, _, w16 = run1
    ref = env.ref(b, VO[b])
    other = env.ref(b, (VO[b] + 1) % 3)
    assert f32[b].shape == ref.shape == (1, 1, F1[b] * env.cfg.hop + 30)
    e_own, e_other = rms(f32[b] - ref), rms(f32[b] - other)
    e16 = rms((w16[b].astype(np.float64) - _ref_i16(ref)) / 32767.0)
    print(f"item {b} (F = {F1[b]}, voice {VO[b]}): fp32 rms vs its voice {e_own:.3e}, vs voice {(VO[b] + 1) % 3} {e_other:.3e}; f16 int16 rms {e16:.3e}")
    assert e_own < 1e-5, (b, e_own)
    assert e_other > 1e-2, (b, e_other)
    assert e16 < 2e-2, (b, e16)
    assert w32[b].dtype == np.int16 and w32[b].shape == ref.shape


def test_golden_latent_with_the_golden_voice(env, run1):
    """Item 4 is the fixture's latent.  The issue lists voice_of = (2, 0, 1, 0, 2, 1) AND asks for item 4 with voice 0 (the fixture's
    conditioning) within 3 LSB of the reference wrapper's wav_i16: the two cannot hold in one call, so the same six latents run a
    second time with item 4 moved to voice 0 and the others as before.  Both calls are held to the oracle."""
    w32, f32, w32g, f32g, _ = run1
    g = env.g
    assert w32g[4].shape == g["wav_i16"].shape
    d = int(np.abs(w32g[4].astype(np.int32) - g["wav_i16"].astype(np.int32)).max())
    e = rms(f32g[4] - env.ref(4, 0))
    print(f"golden latent, voice 0 inside the mixed batch: max |int16 - wav_i16| = {d} LSB, fp32 rms vs oracle {e:.3e}")
    assert d <= 3 and e < 1e-5
    for b in (0, 1, 2, 3, 5):                        # only item 4's row of the table changed
        assert np.array_equal(f32g[b], f32[b]) and np.array_equal(w32g[b], w32[b]), b
    assert rms(f32g[4] - f32[4]) > 1e-2


# ---- 2. isolation, bit for bit ----------------------------------------------------------------------------------------------------
def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_mixed_batch_equals_one_voice_batches_bitwise(env, dtype):
    """Same B and Fmax, so the same launches: only the bias rows differ.  Item b of the mixed batch == item b of
    run_latent_ragged with voice voice_of[b] for everyone; a table of three with voice_of all 1 == run_latent_ragged with voice 1;
    permuting the table's rows with voice_of permuted to match changes nothing."""
    v = env.voc(dtype)
    lats = [_lat(F, 400 + b) for b, F in enumerate(MIX)]
    voices = env.voices[:3]
    w, wf = v.run_latent_voices(lats, voices, VO, return_float=True)
    one = [v.run_latent_ragged(lats, voices[k], return_float=True) for k in range(3)]
    for b in range(len(MIX)):
        assert np.array_equal(w[b], one[VO[b]][0][b]), (dtype, b)
        assert np.array_equal(wf[b], one[VO[b]][1][b]), (dtype, b, rms(wf[b] - one[VO[b]][1][b]))
        for k in range(3):
            if k != VO[b]:                           # ... and the voices are far enough apart for that to mean something
                assert not np.array_equal(wf[b], one[k][1][b]), (dtype, b, k)
    all1 = v.run_latent_voices(lats, voices, [1] * len(MIX), return_float=True)
    assert _same(all1[0], one[1][0]) and _same(all1[1], one[1][1])
    perm = (2, 0, 1)                                 # new row r holds old voice perm[r]
    inv = {old: new for new, old in enumerate(perm)}
    wp = v.run_latent_voices(lats, [voices[p] for p in perm], [inv[x] for x in VO], return_float=True)
    assert _same(wp[0], w) and _same(wp[1], wf)


# ---- 3. every instantiation that can carry the table ------------------------------------------------------------------------------
def _profiled(fn):
    _lib.prof_reset(); _lib.prof_enable(("conv_gemm",))
    try:
        out = fn()
    finally:
        _lib.prof_enable(())
    return out, {k["kernel"] for k in _lib.prof_kernels() if k["launches"] > 0}


def _carriers(kernels):
    return {k[: -len(ITEM_BIAS)] for k in kernels if k.endswith(ITEM_BIAS)}


def _held_to_one_voice(v, lats, voices, vo):
    """a mixed batch, profiled, held bit for bit to its one-voice batches (as test 2); returns (int16, float, kernels)"""
    (w, wf), ks = _profiled(lambda: v.run_latent_voices(lats, voices, vo, return_float=True))
    for k in sorted(set(vo)):
        ow, of = v.run_latent_ragged(lats, voices[k], return_float=True)
        for b in range(len(lats)):
            if vo[b] == k:
                assert np.array_equal(w[b], ow[b]) and np.array_equal(wf[b], of[b]), (b, k)
    assert all(k.endswith(" + lengths") or k.endswith(ITEM_BIAS) for k in ks), sorted(ks)      # a ragged forward: length-aware launches only
    return w, wf, ks


def test_every_length_aware_instantiation_carries_the_table(env, run1):
    """The planner's choices for conv_pre (N = 1536, K = 8960) and the six upsamplers (N = 3072 ... 48) under lengths, by the
    dispatch in gemm_conv.hip with default options.  16-bit: the 64x64 and 128x128 LDS-DMA kernels, the four-stage ring, the 8-wave
    256x192 and 256x128 tiles, the register-staged 128x64 kernel (N = 48); fp32: the 64x64 and 128x128 LDS-DMA kernels and the
    register-staged 128x64 one.  The shapes of tests 1 - 2 reach all but three: 256x192 needs a batch past the big-tile switch (BIG),
    256x128 a K > 2048 layer with M > 128 and fewer than 32 256-row tiles (B = 2, Fmax = 130), the fp32 128x128 kernel >= 1024 tiles
    in one launch (stage 4 at B = 4, Fmax = 128).  With gemm_use_dma = 0 every N > 64 layer lands on the register-staged 128x128
    kernel: covered too.  Every such launch must be one that reads its bias by item, and every result is held to the one-voice
    batches bit for bit."""
    seen = {}
    voices = env.voices
    # the shapes of tests 1 - 2
    for dtype in ("f32", "f16", "bf16"):
        v = env.voc(dtype)
        _, ks1 = _profiled(lambda: v.run_latent_voices(env.lat1, voices[:3], VO))
        _, ks2 = _profiled(lambda: v.run_latent_voices([_lat(F, 400 + b) for b, F in enumerate(MIX)], voices[:3], VO))
        seen[dtype] = _carriers(ks1) | _carriers(ks2)
    # f16, past the big-tile switch: B = 8 at Fmax = 520, four voices
    v = env.voc("f16")
    big = [_lat(F, 500 + b) for b, F in enumerate(BIG)]
    big[1], big[2], big[5] = env.lat1[0], env.lat1[1], env.lat1[3]         # F = 12, 5, 1 with their voices of test 1: the oracle is shared
    w, wf, ks = _held_to_one_voice(v, big, voices, BIG_VO)
    seen["f16"] |= _carriers(ks)
    assert "conv_gemm_dma3_kernel<_Float16, _Float16, 256, 192, 64, 96, 2, true>" in _carriers(ks), sorted(ks)
    for b, b1 in ((1, 0), (2, 1), (5, 3)):
        assert BIG[b] <= 12 and BIG_VO[b] == VO[b1]
        e16 = rms((w[b].astype(np.float64) - _ref_i16(env.ref(b1, VO[b1]))) / 32767.0)
        print(f"big batch item {b} (F = {BIG[b]}, voice {BIG_VO[b]}): f16 int16 rms vs oracle {e16:.3e}")
        assert e16 < 2e-2, (b, e16)
    # the smallest shapes that reach what is left
    _, _, ks = _held_to_one_voice(v, [_lat(130, 600), _lat(3, 601)], voices[:2], (1, 0))
    seen["f16"] |= _carriers(ks)
    _, _, ks = _held_to_one_voice(env.voc("f32"), [_lat(F, 610 + b) for b, F in enumerate((128, 1, 2, 3))], voices[:2], (1, 0, 0, 1))
    seen["f32"] |= _carriers(ks)
    saved = _lib.get_option("gemm_use_dma")
    try:
        _lib.set_option("gemm_use_dma", 0)
        for dtype in ("f32", "f16"):
            _, _, ks = _held_to_one_voice(env.voc(dtype), [_lat(F, 620 + b) for b, F in enumerate((5, 1, 3))], voices[:2], (1, 0, 1))
            seen[dtype] |= _carriers(ks)
    finally:
        _lib.set_option("gemm_use_dma", saved)
    for dtype in ("f32", "f16", "bf16"):
        print(f"{dtype}: instantiations that ran with a per-item bias table:")
        for k in sorted(seen[dtype]):
            print("   ", k)

    def want16(t):
        return {f"conv_gemm_kernel<{t}, {t}, 128, 64, 2, 2, KC>",
                f"conv_gemm_dma_kernel<{t}, {t}, false, 2, 64>",
                f"conv_gemm_dma_kernel<{t}, {t}, false, 4>",
                f"conv_gemm_dma_kernel<{t}, {t}, false>"}
    assert want16("__bf16") <= seen["bf16"], sorted(seen["bf16"])
    assert want16("_Float16") | {"conv_gemm_dma3_kernel<_Float16, _Float16, 256, 192, 64, 96, 2, true>",
                                 "conv_gemm_dma3_kernel<_Float16, _Float16, 256, 128, 64, 64, 3>",
                                 "conv_gemm_kernel<_Float16, _Float16, 128, 128, 2, 2, KC>"} <= seen["f16"], sorted(seen["f16"])
    assert {"conv_gemm_kernel<float, float, 128, 64, 2, 2, KC>", "conv_gemm_dma_kernel<float, float, false, 2, 64>",
            "conv_gemm_dma_kernel<float, float, false>", "conv_gemm_kernel<float, float, 128, 128, 2, 2, KC>"} <= seen["f32"], sorted(seen["f32"])


# ---- 4. device-resident form ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_device_resident_form(env, dtype):
    import torch
    dev = torch.device("cuda", 0)
    v = env.voc(dtype)
    lats = [_lat(F, 400 + b) for b, F in enumerate(MIX)]
    voices = env.voices[:3]
    host = v.run_latent_voices(lats, voices, VO)
    table, _ = BV.voices_table(env.cfg, voices, VO, len(lats))
    lat_cat = torch.from_numpy(np.ascontiguousarray(np.concatenate(lats))).to(dev)
    tab = torch.from_numpy(table).to(dev)
    tcs = [x.shape[0] for x in lats]
    wav, lens = v.run_latent_voices_torch(lat_cat, tcs, tab, VO)
    assert lens == [x.shape[-1] for x in host]
    assert np.array_equal(wav.cpu().numpy(), np.concatenate([x.reshape(-1) for x in host]))
    # other voices, same latents, same handle: nothing is kept from the call before
    vo2 = [(x + 1) % 3 for x in VO]
    wav2, _ = v.run_latent_voices_torch(lat_cat, tcs, tab, vo2)
    host2 = v.run_latent_voices(lats, voices, vo2)
    assert np.array_equal(wav2.cpu().numpy(), np.concatenate([x.reshape(-1) for x in host2]))
    assert not np.array_equal(wav2.cpu().numpy(), wav.cpu().numpy())
    tab2 = tab.flip(0).contiguous()                  # ... and another table at the same address pattern of calls
    wav3, _ = v.run_latent_voices_torch(lat_cat, tcs, tab2, [2 - x for x in VO])
    assert np.array_equal(wav3.cpu().numpy(), wav.cpu().numpy())
    with pytest.raises(ValueError):
        v.run_latent_voices_torch(lat_cat, tcs, tab, [3] + list(VO[1:]))
    with pytest.raises(ValueError):
        v.run_latent_voices_torch(lat_cat, tcs, tab[:, :-1].contiguous(), VO)


def test_table_buffer_grows_without_stale_rows(env):
    """A handle that has just run a larger batch (more items, other voices) gives the bits of a fresh handle."""
    small = [_lat(F, 700 + b) for b, F in enumerate((7, 2, 4))]
    large = [_lat(F, 710 + b) for b, F in enumerate((9, 3, 11, 1, 6, 2, 5, 8))]
    used = env.voc("f32")
    used.run_latent_voices(large, env.voices, (3, 1, 2, 0, 3, 2, 1, 0))
    dirty = used.run_latent_voices(small, env.voices[:2], (1, 0, 1), return_float=True)
    fresh = BV.BigVGANVocoder(env.cfg, env.st, dtype="f32")
    try:
        clean = fresh.run_latent_voices(small, env.voices[:2], (1, 0, 1), return_float=True)
    finally:
        fresh.close()
    assert _same(dirty[0], clean[0]) and _same(dirty[1], clean[1])
    assert all(np.all(np.isfinite(x)) for x in dirty[1])


# ---- 5. errors leave the handle usable --------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_handle_usable(env):
    v = env.voc("f32")
    L = _lib.load()
    lats = [_lat(4, 800), _lat(2, 801)]
    voices = env.voices[:2]
    before = v.run_latent_voices(lats, voices, (1, 0))
    table, _ = BV.voices_table(env.cfg, voices, (1, 0), 2)
    x = np.ascontiguousarray(np.concatenate(lats), np.float32)
    tc = np.asarray([6, 4], np.int64)
    out = np.zeros(8 * env.cfg.hop, np.int16)
    lens = np.zeros(2, np.int64)

    def call(h=None, B=2, t_codes=tc, n_voices=2, n_conds=table.shape[1], voice_of=(1, 0), cap=out.size):
        vo = np.asarray(voice_of, np.int32)
        return L.mi_bigvgan_forward_latent_voices(v._h if h is None else h, B, x.ctypes.data, t_codes.ctypes.data, n_voices,
                                                  table.ctypes.data, n_conds, vo.ctypes.data, out.ctypes.data, None, cap,
                                                  lens.ctypes.data, _lib.MI_HOST)
    assert call(voice_of=(2, 0)) == MI_EINVAL                                # voice index past the table
    assert call(voice_of=(0, -1)) == MI_EINVAL                               # ... and below it
    assert call(n_voices=0, voice_of=(0, 0)) == MI_EINVAL                    # no voice
    assert call(n_conds=table.shape[1] - 1) == MI_EINVAL                     # not the handle's total
    assert call(B=0) == MI_EINVAL                                            # what the ragged entry rejects: no item,
    assert call(t_codes=np.asarray([6, 2], np.int64)) == MI_EINVAL           # fewer than 3 latent rows,
    assert call(cap=6 * env.cfg.hop + 59) == MI_EINVAL                       # out_cap one below the sum
    mel = BigVGANConfig.small()
    m = BV.BigVGANVocoder(mel, W.synth_state(W.bigvgan_spec(mel), 9527), dtype="f32")
    try:
        assert call(h=m._h) == MI_EINVAL                                     # not a graph-F handle
        with pytest.raises(ValueError):
            m.run_latent_voices(lats, voices, (1, 0))
    finally:
        m.close()
    with pytest.raises(ValueError):
        v.run_latent_voices(lats, voices, (2, 0))
    with pytest.raises(ValueError):
        v.run_latent_voices(lats, [], (0, 0))
    with pytest.raises(ValueError):
        v.run_latent_voices(lats, [voices[0], voices[1][:-1] + [voices[1][-1][:-1]]], (1, 0))
    assert call() == MI_OK and lens.tolist() == [4 * env.cfg.hop + 30, 2 * env.cfg.hop + 30]
    assert np.array_equal(out[: int(lens.sum())], np.concatenate([w.reshape(-1) for w in before]))
    assert _same(v.run_latent_voices(lats, voices, (1, 0)), before)
