"""GPU: vocoder windows with halo frames (include/mi355tts.h mi_bigvgan_forward_latent_windows; BigVGANVocoder.run_latent_windows /
run_latent_windows_torch).  The forward is the ragged graph-F one with the windows' first rows as the row-offset table; the new
device code is conv_post's windowed instantiation, which writes only the samples a window keeps.

That the structural halo is SUFFICIENT is proved on the CPU (tests/test_bigvgan_windows_layout.py, bit for bit); these tests prove
indices, trimming and plumbing, where an error is large (a missing halo costs 4e-2 rms).  Gates are the project's own for graph F:
fp32 float output rms < 1e-5, f16 int16 rms / 32767 < 2e-2.
"""
import numpy as np
import pytest

import test_bigvgan_windows_layout as WL
from mi355tts import _lib
from mi355tts import weights as W
from mi355tts import bigvgan as BV
from mi355tts.config import BigVGANConfig
from oracle import bigvgan_np as O

pytestmark = pytest.mark.gpu

MI_OK, MI_EINVAL = 0, -1
F, CUTS = 100, (0, 1, 17, 50, 51, 100)
MIX = (12, 5, 9, 1, 65, 64)
VO = (2, 0, 1, 0, 2, 1)
rms = WL.rms


class Env:
    def __init__(self, cfg):
        self.cfg = cfg
        self.st = W.synth_state(W.bigvgan_spec(cfg), 9527)
        self.voices = [WL.voice(cfg, 100 * (v + 1)) for v in range(3)]
        self.vocs = {}

    def voc(self, dtype):
        if dtype not in self.vocs:
            self.vocs[dtype] = BV.BigVGANVocoder(self.cfg, self.st, dtype=dtype)
        return self.vocs[dtype]

    def lat(self, F_, seed):
        return W.synth_normal(seed, "lat", (F_ + 2, self.cfg.num_mels), std=1.0)

    def close(self):
        for v in self.vocs.values():
            v.close()


@pytest.fixture(scope="module")
def small():
    e = Env(WL.small_f())
    e.lat0 = e.lat(F, 11)
    e.full = O.indextts_f_float(e.cfg, e.st, e.lat0, e.voices[0]).reshape(-1)       # computed once, shared, never written to
    e.full.setflags(write=False)
    yield e
    e.close()


@pytest.fixture(scope="module")
def real():
    e = Env(BigVGANConfig.indextts())
    yield e
    e.close()


def _ranges(cfg, F_, cuts):
    """the samples of the sentence that piece [a, b) owns"""
    return [((a * cfg.hop + 15 if a else 0), (b * cfg.hop + 15 if b < F_ else F_ * cfg.hop + 30)) for a, b in zip(cuts[:-1], cuts[1:])]


def test_five_windows_fp32_against_the_oracle_and_the_engine(small):
    """F = 100 cut at 0/1/17/50/51/100 with the structural halo (39): first kept samples at 15 mod 256 (window 1: 8 + 15) and
    elsewhere (39 * 8 + 15), kept ranges shorter than one 256-sample workgroup (23, 128 and 8 samples), float and int16 outputs."""
    cfg, v = small.cfg, small.voc("f32")
    H = cfg.halo_frames()
    assert H == 39
    wins = WL.cut_windows(F, CUTS, H)
    first, lens, offs, _ = BV.window_layout(cfg, F, wins)
    assert 23 in first and 39 * 8 + 15 in first and min(lens) < 256
    w, wf = v.run_latent_windows(small.lat0[:F], wins, small.voices[:1], [0] * len(wins), return_float=True)
    assert [x.size for x in w] == lens and [x.size for x in wf] == lens
    ew, ef = v.run_latent_ragged([small.lat0], small.voices[0], return_float=True)
    ew, ef = ew[0].reshape(-1), ef[0].reshape(-1)
    for p, (s0, s1) in zip(wf, _ranges(cfg, F, CUTS)):
        e = rms(p - small.full[s0:s1])
        print(f"piece [{s0}, {s1}): fp32 rms vs the oracle's slice {e:.3e}")
        assert p.size == s1 - s0 and e < 1e-5
    cat, cat_i = np.concatenate(wf), np.concatenate(w)
    assert cat.shape == ef.shape
    e_eng = rms(cat - ef)
    e_i16 = rms((cat_i.astype(np.float64) - ew) / 32767.0)
    print(f"concatenation vs the engine's whole-sentence forward: fp32 rms {e_eng:.3e}, int16 rms {e_i16:.3e}")
    assert e_eng < 1e-5 and e_i16 < 1e-4
    # the int16 output is the float one converted: trunc(clamp(v * 32767))
    assert np.array_equal(cat_i, np.clip(cat * np.float32(32767.0), -32768.0, 32767.0).astype(np.int16))
    # halo 0: the same cuts, every piece alone and untrimmed; the host keeps each piece's own samples.  Far outside the gate.
    w0, wf0 = v.run_latent_windows(small.lat0[:F], WL.cut_windows(F, CUTS, 0), small.voices[:1], [0] * len(wins), return_float=True)
    kept = [p[15 if a else 0: p.size - (15 if b < F else 0)] for p, (a, b) in zip(wf0, zip(CUTS[:-1], CUTS[1:]))]
    e0 = rms(np.concatenate(kept) - ef)
    print(f"halo 0: rms {e0:.3e}")
    assert e0 > 1e-3


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_untrimmed_windows_are_the_voices_forward_bitwise(small, dtype):
    """head = tail = 0 over whole sentences minus their last two rows == run_latent_voices, bit for bit"""
    v = small.voc(dtype)
    lats = [small.lat(f, 400 + b) for b, f in enumerate(MIX)]
    w, wf = v.run_latent_voices(lats, small.voices, VO, return_float=True)
    cat = np.concatenate(lats)
    wins, r = [], 0
    for f in MIX:
        wins.append((r, f, 0, 0))
        r += f + 2
    ww, wwf = v.run_latent_windows(cat, wins, small.voices, VO, return_float=True)
    for b in range(len(MIX)):
        np.testing.assert_array_equal(ww[b], w[b].reshape(-1))
        np.testing.assert_array_equal(wwf[b], wf[b].reshape(-1))


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_real_config_windows(real, dtype):
    """BigVGANConfig.indextts(), halo 34: one sentence of F = 80 cut at 0/9/40/80, against the engine's own whole-sentence forward"""
    cfg, v = real.cfg, real.voc(dtype)
    assert cfg.halo_frames() == 34
    Fr, cuts = 80, (0, 9, 40, 80)
    lat = real.lat(Fr, 21)
    ew, ef = v.run_latent_ragged([lat], real.voices[1], return_float=True)
    w, wf = v.run_latent_windows(lat[:Fr], WL.cut_windows(Fr, cuts, 34), real.voices[:2], [1, 1, 1], return_float=True)
    cat, cat_i = np.concatenate(wf), np.concatenate(w)
    assert cat.shape == ef[0].reshape(-1).shape
    e32 = rms(cat - ef[0].reshape(-1))
    e16 = rms((cat_i.astype(np.float64) - ew[0].reshape(-1)) / 32767.0)
    print(f"{dtype}: windows vs the whole sentence: float rms {e32:.3e}, int16 rms {e16:.3e}")
    if dtype == "f32":
        assert e32 < 1e-5
    assert e16 < 2e-2


def test_two_sentences_two_voices_overlapping_rows_device(small):
    """windows of two sentences and two voices in one call, overlapping rows of one device tensor shaped like a queue session's
    (n, cap, hidden) `hidden`; an output tensor larger than the kept samples keeps its sentinel outside them"""
    import torch
    cfg, v = small.cfg, small.voc("f32")
    dev = torch.device("cuda", 0)
    H = cfg.halo_frames()
    Fs, cap = (100, 61), 110
    lats = [small.lat0, small.lat(Fs[1], 31)]
    hid = np.zeros((2, cap, cfg.num_mels), np.float32)
    for i, x in enumerate(lats):
        hid[i, : x.shape[0]] = x
    full = v.run_latent_voices(lats, small.voices, (0, 2), return_float=True)[1]
    pieces = [(0, 0, 30), (1, 0, 20), (0, 30, 70), (1, 20, 61), (0, 70, 100)]            # (sentence, a, b), interleaved
    wins, vo = [], []
    for i, a, b in pieces:
        lo, hi = max(0, a - H), min(Fs[i], b + H)
        wins.append((i * cap + lo, hi - lo, a - lo, hi - b))
        vo.append((0, 2)[i])
    table, _ = BV.voices_table(cfg, small.voices, vo, len(wins))
    _, lens, offs, _ = BV.window_layout(cfg, 2 * cap, wins)
    n = sum(lens)
    out = torch.full((n + 300,), -12345, dtype=torch.int16, device=dev)
    outf = torch.full((n + 300,), -7.0, dtype=torch.float32, device=dev)
    wav, got_lens = v.run_latent_windows_torch(torch.from_numpy(hid).to(dev), wins, torch.from_numpy(table).to(dev), vo, out=out,
                                               out_float=outf)
    assert got_lens == lens
    o, of = out.cpu().numpy(), outf.cpu().numpy()
    assert np.all(o[n:] == -12345) and np.all(of[n:] == -7.0)                # the canary
    assert np.all(of[:n] != -7.0)
    for (i, a, b), off, ln in zip(pieces, offs, lens):
        s0 = a * cfg.hop + 15 if a else 0
        s1 = b * cfg.hop + 15 if b < Fs[i] else Fs[i] * cfg.hop + 30
        assert ln == s1 - s0
        e = rms(of[off:off + ln] - full[i].reshape(-1)[s0:s1])
        print(f"sentence {i} frames [{a}, {b}): rms vs its whole forward {e:.3e}")
        assert e < 1e-5
    # a window of the other sentence with this voice is far away: the voice index reaches the right rows of the table
    assert rms(of[offs[1]:offs[1] + lens[1]] - v.run_latent_voices(lats[1:], small.voices, (0,), return_float=True)[1][0].reshape(-1)[:lens[1]]) > 1e-3
    with pytest.raises(ValueError):
        v.run_latent_windows_torch(torch.from_numpy(hid).to(dev), wins, torch.from_numpy(table).to(dev), vo, out=out[: n - 1])


def test_argument_errors_leave_the_handle_usable(small):
    cfg, v = small.cfg, small.voc("f32")
    L = _lib.load()
    lat = np.ascontiguousarray(small.lat0[:30])
    wins = [(0, 20, 0, 5), (10, 20, 5, 0)]
    before, before_f = v.run_latent_windows(lat, wins, small.voices[:2], (1, 0), return_float=True)
    table, _ = BV.voices_table(cfg, small.voices[:2], (1, 0), 2)
    _, lens0, _, _ = BV.window_layout(cfg, 30, wins)
    out = np.zeros(sum(lens0), np.int16)
    lens = np.zeros(2, np.int64)

    def call(h=None, B=2, rows_total=30, row0=(0, 10), rows=(20, 20), head=(0, 5), tail=(5, 0), n_voices=2, n_conds=table.shape[1],
             voice_of=(1, 0), cap=out.size):
        a = [np.asarray(x, np.int64) for x in (row0, rows)] + [np.asarray(x, np.int32) for x in (head, tail, voice_of)]
        return L.mi_bigvgan_forward_latent_windows(v._h if h is None else h, B, lat.ctypes.data, rows_total, a[0].ctypes.data,
                                                   a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, n_voices, table.ctypes.data,
                                                   n_conds, a[4].ctypes.data, out.ctypes.data, None, cap, lens.ctypes.data, _lib.MI_HOST)
    assert call(B=0) == MI_EINVAL
    assert call(rows=(20, 0), head=(0, 0), tail=(5, 0)) == MI_EINVAL          # rows < 1
    assert call(head=(-1, 5)) == MI_EINVAL and call(tail=(5, -1)) == MI_EINVAL
    assert call(head=(15, 5)) == MI_EINVAL                                    # head + tail >= rows
    assert call(row0=(-1, 10)) == MI_EINVAL and call(row0=(0, 11)) == MI_EINVAL and call(rows_total=29) == MI_EINVAL
    assert call(rows_total=1 << 29, rows=(20, 1 << 27)) == MI_EINVAL          # past the ragged path's frame limit
    assert call(cap=out.size - 1) == MI_EINVAL
    assert call(voice_of=(2, 0)) == MI_EINVAL and call(voice_of=(0, -1)) == MI_EINVAL
    assert call(n_voices=0, voice_of=(0, 0)) == MI_EINVAL
    assert call(n_conds=table.shape[1] - 1) == MI_EINVAL
    mel = BigVGANConfig.small()
    m = BV.BigVGANVocoder(mel, W.synth_state(W.bigvgan_spec(mel), 9527), dtype="f32")
    try:
        assert call(h=m._h) == MI_EINVAL                                      # not a graph-F handle
        with pytest.raises(ValueError):
            m.run_latent_windows(lat, wins, small.voices[:2], (1, 0))
    finally:
        m.close()
    with pytest.raises(ValueError):
        v.run_latent_windows(lat, [(0, 31, 0, 0)], small.voices[:2], (1,))
    assert call() == MI_OK and lens.tolist() == lens0
    assert np.array_equal(out, np.concatenate(before))
    again, again_f = v.run_latent_windows(lat, wins, small.voices[:2], (1, 0), return_float=True)
    assert all(np.array_equal(x, y) for x, y in zip(again, before)) and all(np.array_equal(x, y) for x, y in zip(again_f, before_f))
