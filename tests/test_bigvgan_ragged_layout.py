"""CPU: host plan of ragged BigVGAN batches (mi355tts.bigvgan.ragged_layout) for both vocoder forms, the checks the
engine would refuse with, and the C-ABI exports of the ragged entries (no GPU needed)."""
import pytest

from mi355tts import _lib
from mi355tts.bigvgan import ragged_layout
from mi355tts.config import BigVGANConfig


def test_mel_layout_offsets_and_lengths():
    cfg = BigVGANConfig()
    F, in_offs, out_lens, out_offs, Fmax = ragged_layout(cfg, [12, 5, 9, 1, 65, 64])
    assert F == [12, 5, 9, 1, 65, 64] and Fmax == 65
    assert in_offs == [0, 12, 17, 26, 27, 92]
    assert out_lens == [f * 256 + 30 for f in F]
    assert out_offs[0] == 0 and all(out_offs[b + 1] - out_offs[b] == out_lens[b] for b in range(5))


def test_latent_layout_drops_two_rows():
    cfg = BigVGANConfig.indextts()
    F, in_offs, out_lens, out_offs, Fmax = ragged_layout(cfg, [3, 17, 100], latent=True)
    assert F == [1, 15, 98] and Fmax == 98
    assert in_offs == [0, 3, 20]                                   # latent rows, the dropped two included
    assert out_lens == [f * cfg.hop + 30 for f in F] and out_offs == [0, out_lens[0], out_lens[0] + out_lens[1]]


def test_single_item_is_the_uniform_shape():
    cfg = BigVGANConfig.small()
    F, _, out_lens, out_offs, Fmax = ragged_layout(cfg, [20])
    assert F == [20] and Fmax == 20 and out_offs == [0] and out_lens == [20 * cfg.hop + 30]


@pytest.mark.parametrize("frames,latent", [([], False), ([4, 0], False), ([-1], False), ([3, 2], True), ([], True)])
def test_rejections(frames, latent):
    with pytest.raises(ValueError):
        ragged_layout(BigVGANConfig(), frames, latent=latent)


def test_rejects_frames_past_the_uniform_limit():
    cfg = BigVGANConfig()
    with pytest.raises(ValueError):
        ragged_layout(cfg, [1, (1 << 30) // cfg.hop])
    ragged_layout(cfg, [1, (1 << 30) // cfg.hop - 1])


def test_ragged_entries_exported():
    L = _lib.load()
    for n in ("mi_bigvgan_forward_ragged", "mi_bigvgan_forward_latent_ragged", "mi_f5_synthesize_mel_ragged"):
        assert hasattr(L, n), n
