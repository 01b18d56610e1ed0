"""CPU: vocoder windows with halo frames (BigVGANConfig.halo_frames, bigvgan.window_layout; the engine entry is
mi_bigvgan_forward_latent_windows, held to these on the GPU by tests/test_gpu_bigvgan_windows.py).

  1. halo_frames() is the generator's receptive field, by the interval walk: 34 / 38 / 39 / 39 frames for the four configs;
  2. with that halo the numpy oracle, run window by window and trimmed by window_layout's rule, reproduces the whole sentence's
     waveform with np.array_equal (a tolerance test could not prove a halo sufficient: this does), and without a halo it does not;
  3. window_layout raises ValueError for everything the C entry answers with MI_EINVAL.
"""
import numpy as np
import pytest

from mi355tts import weights as W
from mi355tts import bigvgan as BV
from mi355tts.config import BigVGANConfig
from oracle import bigvgan_np as O


def small_f(num_mels=128):
    """the (4, 2) / (8, 4) graph-F generator of the window tests: hop 8, halo 39"""
    return BigVGANConfig(num_mels=num_mels, upsample_initial_channel=32, upsample_rates=(4, 2), upsample_kernel_sizes=(8, 4),
                         use_bias_at_final=True, pre_layernorm=True, speaker_cond=True)


def thin_ladder():
    """the IndexTTS-1.5 rate ladder (hop 1024, halo 34) with thin channels: 64 -> 1"""
    return BigVGANConfig(num_mels=16, upsample_initial_channel=64, upsample_rates=(4, 4, 4, 4, 2, 2),
                         upsample_kernel_sizes=(8, 8, 4, 4, 4, 4), use_bias_at_final=True, pre_layernorm=True, speaker_cond=True)


def voice(cfg, seed):
    sizes = [cfg.stage_channels(i) for i in range(cfg.num_upsamples)] + [cfg.upsample_initial_channel]
    return [W.synth_normal(seed + i, "cond", (n,), std=0.2) for i, n in enumerate(sizes)]


def cut_windows(F, cuts, halo):
    """pieces [a, b) between consecutive cuts -> (row0, rows, head, tail) with `halo` frames at every cut inside [0, F)"""
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        lo, hi = max(0, a - halo), min(F, b + halo)
        out.append((lo, hi - lo, a - lo, hi - b))
    return out


def rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, np.float64)))))


def test_halo_frames_is_the_receptive_field():
    assert BigVGANConfig.indextts().halo_frames() == 34
    assert BigVGANConfig().halo_frames() == 38
    assert BigVGANConfig.small().halo_frames() == 39
    assert small_f().halo_frames() == 39
    assert thin_ladder().halo_frames() == 34                  # the rates and kernels decide, not the channels


def _oracle_pieces(cfg, st, lat, conds, wins):
    """every window through the oracle alone (two rows appended: indextts_f_float drops the last two), trimmed by window_layout"""
    first, lens, offs, _ = BV.window_layout(cfg, lat.shape[0] - 2, wins)
    pad = np.zeros((2, lat.shape[1]), np.float32)
    out = []
    for (row0, rows, _, _), f0, n in zip(wins, first, lens):
        y = O.indextts_f_float(cfg, st, np.concatenate([lat[row0:row0 + rows], pad]), conds).reshape(-1)
        assert y.size == rows * cfg.hop + 30
        out.append(y[f0:f0 + n])
    assert offs == [int(v) for v in np.cumsum([0] + lens[:-1])]
    return out


@pytest.mark.parametrize("make,F,cuts", [(small_f, 100, (0, 1, 17, 50, 51, 100)), (thin_ladder, 80, (0, 9, 40, 80))],
                         ids=["small-4x2", "indextts-ladder-thin"])
def test_oracle_windows_reproduce_the_sentence_exactly(make, F, cuts):
    cfg = make()
    H = cfg.halo_frames()
    st = W.synth_state(W.bigvgan_spec(cfg), 9527)
    conds = voice(cfg, 100)
    lat = W.synth_normal(11, "lat", (F + 2, cfg.num_mels), std=1.0)
    full = O.indextts_f_float(cfg, st, lat, conds).reshape(-1)
    assert full.size == F * cfg.hop + 30
    pieces = _oracle_pieces(cfg, st, lat, conds, cut_windows(F, cuts, H))
    got = np.concatenate(pieces)
    assert got.shape == full.shape
    assert np.array_equal(got, full), rms(got - full)
    # piece [a, b) holds samples [a ? a * hop + 15 : 0, b < F ? b * hop + 15 : F * hop + 30) of the sentence
    s = 0
    for (a, b), p in zip(zip(cuts[:-1], cuts[1:]), pieces):
        assert s == (a * cfg.hop + 15 if a else 0)
        s += p.size
        assert s == (b * cfg.hop + 15 if b < F else F * cfg.hop + 30)


def test_without_a_halo_the_pieces_are_wrong():
    """The same cuts at halo 0: every piece runs alone (untrimmed, head = tail = 0), the host keeps each piece's own samples.
    The rms error against the whole sentence is far above any gate (4.4e-2 at a signal rms of 0.19 when this was written)."""
    cfg = small_f()
    F, cuts = 100, (0, 1, 17, 50, 51, 100)
    st = W.synth_state(W.bigvgan_spec(cfg), 9527)
    conds = voice(cfg, 100)
    lat = W.synth_normal(11, "lat", (F + 2, cfg.num_mels), std=1.0)
    full = O.indextts_f_float(cfg, st, lat, conds).reshape(-1)
    wins = cut_windows(F, cuts, 0)
    assert all(h == 0 and t == 0 for _, _, h, t in wins)
    pieces = _oracle_pieces(cfg, st, lat, conds, wins)
    kept = []
    for (a, b), p in zip(zip(cuts[:-1], cuts[1:]), pieces):
        assert p.size == (b - a) * cfg.hop + 30           # untrimmed
        kept.append(p[15 if a else 0: p.size - (15 if b < F else 0)])
    got = np.concatenate(kept)
    assert got.shape == full.shape
    e = rms(got - full)
    print(f"halo 0: rms error {e:.3e} at signal rms {rms(full):.3e}")
    assert e > 1e-3


def test_window_layout_values():
    cfg = small_f()
    first, lens, offs, Fmax = BV.window_layout(cfg, 102, [(0, 40, 0, 39), (0, 56, 1, 39), (11, 89, 39, 0), (5, 1, 0, 0)])
    assert first == [0, 8 + 15, 39 * 8 + 15, 0]
    assert lens == [1 * 8 + 15, 16 * 8, 50 * 8 + 15, 8 + 30]
    assert offs == [0, 23, 23 + 128, 23 + 128 + 415] and Fmax == 89


def test_window_layout_errors():
    cfg = small_f()
    ok = [(0, 10, 0, 2), (5, 20, 3, 0)]
    BV.window_layout(cfg, 30, ok)
    for bad in ([],                                    # B < 1
                [(0, 0, 0, 0)],                        # rows < 1
                [(0, 10, -1, 0)], [(0, 10, 0, -1)],    # head or tail < 0
                [(0, 10, 5, 5)], [(0, 1, 1, 0)],       # head + tail >= rows
                [(-1, 10, 0, 0)], [(21, 10, 0, 0)], [(30, 1, 0, 0)],      # outside [0, latent_rows)
                [(0, 10, 0)], [(0, 10, 0, 0.5)]):
        with pytest.raises(ValueError):
            BV.window_layout(cfg, 30, ok + bad if bad else bad)
    with pytest.raises(ValueError):
        BV.window_layout(cfg, 0, ok)
    with pytest.raises(ValueError):                    # past the ragged path's frame limit
        BV.window_layout(cfg, 1 << 28, [(0, 1 << 27, 0, 0)])
    with pytest.raises(ValueError):                    # not a graph-F config
        BV.window_layout(BigVGANConfig.small(), 30, ok)
