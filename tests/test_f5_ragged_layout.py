"""CPU: the host-side plan of a ragged F5 batch (mi355tts.f5.ragged_layout) — per-utterance prompt frames, waveform lengths,
slab height — and the inputs it refuses before anything reaches the GPU."""
import dataclasses

import pytest

from mi355tts.config import F5Config
from mi355tts.f5 import ragged_layout
from mi355tts.text import max_duration


def test_layout_follows_the_front_end_and_graph_c():
    cfg = F5Config()
    L, T, N = [144000, 162240, 89600], [120, 130, 60], [1126, 1268, 700]
    R, F, out, Nmax = ragged_layout(cfg, L, T, N)
    assert R == [cfg.ref_frames(x) for x in L] == [563, 634, 351]
    assert F == [n - r for n, r in zip(N, R)]
    assert out == [(n - r - 1) * cfg.hop_length for n, r in zip(N, R)]
    assert Nmax == 1268


def test_layout_bigvgan_front_end_frames():
    cfg = dataclasses.replace(F5Config(), mel_spec_type="bigvgan")
    R, _, out, _ = ragged_layout(cfg, [144000, 30000], [10, 10], [1000, 200])
    assert R == [cfg.ref_frames(144000), cfg.ref_frames(30000)] == [(144000 - 256) // 256 + 1, (30000 - 256) // 256 + 1]
    assert out == [(1000 - R[0] - 1) * 256, (200 - R[1] - 1) * 256]


def test_layout_one_generated_frame_gives_an_empty_waveform():
    cfg = F5Config()
    R, F, out, Nmax = ragged_layout(cfg, [25600], [5], [cfg.ref_frames(25600) + 1])
    assert F == [1] and out == [0] and Nmax == R[0] + 1


def test_layout_with_the_reference_duration_formula():
    cfg = F5Config()
    ref = "Some call me nature, others call me mother nature."
    gens = ["Hello there.", "A much longer sentence that asks for a lot more generated audio than the first one does."]
    L = [96000, 120000]
    N = [max_duration(l, ref, g) for l, g in zip(L, gens)]
    R, F, out, Nmax = ragged_layout(cfg, L, [len(ref) + len(g) for g in gens], N)
    assert Nmax == max(N) and all(f >= 1 for f in F) and N[0] != N[1]


@pytest.mark.parametrize("L,T,N", [
    ([144000, 144000], [10, 10], [1126, 563]),           # N_u < R_u + 1 (no generated frame)
    ([144000], [10], [563]),
    ([144000], [900], [800]),                            # N_u < T_u
    ([144000], [10], [5000]),                            # N_u > max_signal_length
    ([100], [1], [50]),                                  # prompt shorter than one STFT frame
    ([144000], [-1], [800]),                             # negative text length
    ([], [], []),                                        # U < 1
    ([144000, 144000], [10], [800, 800]),                # length lists disagree
])
def test_layout_refuses_impossible_inputs(L, T, N):
    with pytest.raises(ValueError):
        ragged_layout(F5Config(), L, T, N)
