"""CPU: ``voices_table`` — the host-side model of the argument rules of mi_bigvgan_forward_latent_voices (several voices in one
ragged graph-F forward): the (V, total_cond) float32 table in the flat layout [cond_0 .. cond_{n_up-1}, cond_pre], the int32
voice index per item, and every ValueError the engine's MI_EINVAL stands for.  No GPU, no library.
"""
import numpy as np
import pytest

from mi355tts import weights as W
from mi355tts.bigvgan import flat_conds, voices_table
from mi355tts.config import BigVGANConfig

CFG = BigVGANConfig.indextts()
SIZES = [CFG.stage_channels(i) for i in range(CFG.num_upsamples)] + [CFG.upsample_initial_channel]
TOTAL = sum(SIZES)


def _voice(seed):
    return [W.synth_normal(seed, f"cond{i}", (n,), std=0.2) for i, n in enumerate(SIZES)]


def test_layout_and_dtype():
    assert SIZES == [768, 384, 192, 96, 48, 24, 1536] and TOTAL == 3048
    voices = [_voice(1), _voice(2), _voice(3)]
    tab, idx = voices_table(CFG, voices, (2, 0, 1, 0, 2, 1), 6)
    assert tab.shape == (3, TOTAL) and tab.dtype == np.float32 and tab.flags["C_CONTIGUOUS"]
    assert idx.shape == (6,) and idx.dtype == np.int32 and idx.tolist() == [2, 0, 1, 0, 2, 1]
    for v, conds in enumerate(voices):
        off = 0
        for c in conds:                       # cond_0 .. cond_{n_up-1}, then cond_pre: the order of mi_bigvgan_forward_latent
            assert np.array_equal(tab[v, off:off + c.size], c)
            off += c.size
        assert off == TOTAL
        assert np.array_equal(tab[v], flat_conds(CFG, conds))
    assert np.array_equal(tab[0, -1536:], voices[0][-1])


def test_shapes_the_exporter_hands_over():
    """(1, C, 1) arrays, float64 values and lists are accepted like run_latent accepts them; the index may be any integer type."""
    v = _voice(4)
    shaped = [c.reshape(1, -1, 1).astype(np.float64) for c in v[:3]] + [c.tolist() for c in v[3:]]
    tab, idx = voices_table(CFG, [shaped], np.zeros(2, np.int64), 2)
    assert tab.dtype == np.float32 and np.array_equal(tab[0], flat_conds(CFG, v))
    assert idx.dtype == np.int32 and idx.tolist() == [0, 0]


def test_one_zero_voice_reproduces_flat_conds():
    """V = 1 with zeros is the argument set of the one-voice entry: the table's only row is _flat_conds' vector."""
    from mi355tts.bigvgan import BigVGANVocoder
    zeros = [np.zeros(n, np.float32) for n in SIZES]
    tab, idx = voices_table(CFG, [zeros], [0] * 5, 5)
    v = BigVGANVocoder.__new__(BigVGANVocoder)            # _flat_conds needs the config only: no handle, no GPU
    v.cfg = CFG
    assert tab.shape == (1, TOTAL) and np.array_equal(tab[0], v._flat_conds(zeros)) and not tab.any()
    assert idx.tolist() == [0] * 5
    one = _voice(9)
    assert np.array_equal(voices_table(CFG, [one], [0], 1)[0][0], v._flat_conds(one))


@pytest.mark.parametrize("what", ["no voices", "no items", "index count", "index high", "index negative", "index not an integer",
                                   "vector count", "vector size", "not graph F"])
def test_value_errors(what):
    voices = [_voice(1), _voice(2)]
    cfg, vo, n = CFG, [0, 1, 1], 3
    if what == "no voices":
        voices = []
    elif what == "no items":
        vo, n = [], 0
    elif what == "index count":
        vo = [0, 1]
    elif what == "index high":
        vo = [0, 2, 1]
    elif what == "index negative":
        vo = [0, -1, 1]
    elif what == "index not an integer":
        vo = [0, 0.5, 1]
    elif what == "vector count":
        voices[1] = voices[1][:-1]
    elif what == "vector size":
        voices[1][2] = voices[1][2][:-1]
    elif what == "not graph F":
        cfg = BigVGANConfig()
    with pytest.raises(ValueError):
        voices_table(cfg, voices, vo, n)
    tab, idx = voices_table(CFG, [_voice(1), _voice(2)], [0, 1, 1], 3)            # the valid call next to each of them
    assert tab.shape == (2, TOTAL) and idx.tolist() == [0, 1, 1]


def test_int16_oracle_is_the_float_oracle_quantised():
    """tests/test_gpu_bigvgan_voices.py computes the float oracle once per (item, voice) and derives the int16 oracle of its f16
    gate from it: O.indextts_f_int16 must be O.indextts_f_float followed by clip * 32767 -> int16 (truncation), value for value."""
    from oracle import bigvgan_np as O
    cfg = BigVGANConfig(num_mels=16, upsample_initial_channel=32, upsample_rates=(4, 2), upsample_kernel_sizes=(8, 4),
                        use_bias_at_final=True, pre_layernorm=True, speaker_cond=True)
    st = W.synth_state(W.bigvgan_spec(cfg), 9527)
    lat = W.synth_normal(5, "lat", (9, cfg.num_mels), std=1.0)
    conds = [W.synth_normal(6 + i, "cond", (n,), std=0.2) for i, n in enumerate((16, 8, 32))]
    y = O.indextts_f_float(cfg, st, lat, conds)
    assert np.array_equal(O.indextts_f_int16(cfg, st, lat, conds), (np.clip(y, -1.0, 1.0) * np.float32(32767.0)).astype(np.int16))
    assert np.abs(y).max() > 1e-3
