"""BigVGAN-v2 vocoder: host-side mirror of the reference's BigVGAN graph.

``BigVGANVocoder.run(mel)`` is what ``ort_session_A.run_with_ort_values([generated_wav],
{mel_features: ...})`` does in /root/reference BigVGAN/Export_BigVGAN.py:165-175 — mel
(1, 100, F) float32 in, int16 (1, 1, 256*F + 30) out — executed by hand-written gfx950 kernels
through the C-ABI.  B > 1 is this engine's extension (the reference graph is batch-1).
"""
from __future__ import annotations

import operator
from typing import Optional

import numpy as np

from . import _lib
from .config import BigVGANConfig
from .weights import pack_bigvgan


def ragged_layout(cfg: BigVGANConfig, frames, latent: bool = False):
    """Host-side plan of a ragged batch (BigVGANVocoder.run_ragged / run_latent_ragged): per item the frames F_b, the offset of
    its input in the concatenated input (frames for mels, latent rows for graph F), its waveform length F_b * hop + 30 and
    offset in the concatenated output, and the slab height Fmax = max F_b.  `frames` are the mel frames, or with latent=True
    the latent rows T_b (F_b = T_b - 2, the reference drops the last two).  Raises ValueError for inputs the engine would
    refuse, before the GPU is touched.  Returns (F, in_offs, out_lens, out_offs, Fmax)."""
    n = [int(x) for x in frames]
    if not n:
        raise ValueError("ragged batch: at least one item")
    lo = 3 if latent else 1
    for b, x in enumerate(n):
        if x < lo:
            raise ValueError(f"item {b}: {x} {'latent rows' if latent else 'frames'}, needs >= {lo}")
    F = [x - 2 for x in n] if latent else n
    Fmax = max(F)
    if Fmax * cfg.hop >= 1 << 30:
        raise ValueError(f"ragged batch: {Fmax} frames exceed the vocoder's limit")
    in_offs = [int(v) for v in np.concatenate([[0], np.cumsum(n)[:-1]])]
    out_lens = [f * cfg.hop + 30 for f in F]
    out_offs = [int(v) for v in np.concatenate([[0], np.cumsum(out_lens)[:-1]])]
    return F, in_offs, out_lens, out_offs, Fmax


def window_layout(cfg: BigVGANConfig, latent_rows: int, windows):
    """Host-side plan of a windowed graph-F forward (BigVGANVocoder.run_latent_windows, mi_bigvgan_forward_latent_windows).
    windows = (row0, rows, head, tail) each: frames [row0, row0 + rows) of a (latent_rows, gpt_dim) array, of which `head`
    leading and `tail` trailing frames are halo.  Run alone the window gives rows * hop + 30 samples; the kept ones are
    [first, first + out_len) with first = head * hop + 15 (0 without a head) and the end at (rows - tail) * hop + 15
    (rows * hop + 30 without a tail).  Raises ValueError where the engine says MI_EINVAL, before the GPU is touched.
    Returns (first, out_lens, out_offs, Fmax): per window the first kept sample, the kept count and its offset in the
    concatenated output, and the slab height."""
    if not (cfg.pre_layernorm and cfg.speaker_cond):
        raise ValueError("this config is not an IndexTTS graph-F vocoder (no latent input)")
    try:
        n_rows = operator.index(latent_rows)
        win = [tuple(operator.index(v) for v in w) for w in windows]
    except TypeError:
        raise ValueError("latent_rows and the windows must hold integers") from None
    if not win:
        raise ValueError("windows: at least one window")
    if n_rows < 1:
        raise ValueError("latent_rows must be >= 1")
    first, out_lens = [], []
    for b, w in enumerate(win):
        if len(w) != 4:
            raise ValueError(f"window {b}: expected (row0, rows, head, tail)")
        row0, rows, head, tail = w
        if rows < 1:
            raise ValueError(f"window {b}: {rows} rows, needs >= 1")
        if head < 0 or tail < 0 or head + tail >= rows:
            raise ValueError(f"window {b}: head {head} and tail {tail} must be >= 0 and leave a frame of {rows} rows")
        if row0 < 0 or row0 + rows > n_rows:
            raise ValueError(f"window {b}: rows [{row0}, {row0 + rows}) lie outside [0, {n_rows})")
        if rows * cfg.hop >= 1 << 30:
            raise ValueError(f"window {b}: {rows} frames exceed the vocoder's limit")
        lo = head * cfg.hop + 15 if head else 0
        hi = (rows - tail) * cfg.hop + 15 if tail else rows * cfg.hop + 30
        first.append(lo)
        out_lens.append(hi - lo)
    out_offs = [int(v) for v in np.concatenate([[0], np.cumsum(out_lens)[:-1]])]
    return first, out_lens, out_offs, max(w[1] for w in win)


def flat_conds(cfg: BigVGANConfig, conds) -> np.ndarray:
    """One voice's conditioning vectors [cond_0 .. cond_{n-1}, cond_pre] (each (1, C, 1) / (C,)) as the flat float32 row the
    C-ABI takes (mi_bigvgan_forward_latent).  ValueError for a wrong count or size."""
    want = [cfg.stage_channels(i) for i in range(cfg.num_upsamples)] + [cfg.upsample_initial_channel]
    conds = list(conds)
    if len(conds) != len(want):
        raise ValueError(f"expected {len(want)} conditioning vectors")
    flat = []
    for c, n in zip(conds, want):
        c = np.asarray(c, dtype=np.float32).reshape(-1)
        if c.size != n:
            raise ValueError(f"conditioning vector has {c.size} values, expected {n}")
        flat.append(c)
    return np.ascontiguousarray(np.concatenate(flat))


def voices_table(cfg: BigVGANConfig, voices, voice_of, n_items: int):
    """Host-side arguments of a several-voice graph-F forward (BigVGANVocoder.run_latent_voices, mi_bigvgan_forward_latent_voices):
    voices = V >= 1 conditioning lists as ``run_latent`` takes them, voice_of = the voice index of each of the n_items items.
    Returns (table, index): float32 (V, total_cond), row v = voice v flattened like ``flat_conds``, and int32 (n_items,).
    Raises ValueError for what the engine would refuse (no voice, no item, a count or size that does not fit the config, an
    index outside [0, V)), before the GPU is touched."""
    if not (cfg.pre_layernorm and cfg.speaker_cond):
        raise ValueError("this config is not an IndexTTS graph-F vocoder (no speaker conditioning)")
    voices = list(voices)
    if not voices:
        raise ValueError("voices: at least one voice")
    rows = []
    for v, conds in enumerate(voices):
        try:
            rows.append(flat_conds(cfg, conds))
        except ValueError as e:
            raise ValueError(f"voice {v}: {e}") from None
    if int(n_items) < 1:
        raise ValueError("ragged batch: at least one item")
    try:
        index = [operator.index(x) for x in voice_of]
    except TypeError:
        raise ValueError("voice_of must hold integers") from None
    if len(index) != int(n_items):
        raise ValueError(f"voice_of has {len(index)} entries for {int(n_items)} items")
    for b, x in enumerate(index):
        if not 0 <= x < len(rows):
            raise ValueError(f"item {b}: voice {x} is outside [0, {len(rows)})")
    return np.ascontiguousarray(np.stack(rows), dtype=np.float32), np.asarray(index, dtype=np.int32)


class BigVGANVocoder:
    def __init__(self, cfg: BigVGANConfig, state: Optional[dict] = None, *, blob: Optional[np.ndarray] = None,
                 blob_device=None, dtype: str = "f32", device: int = 0):
        self.cfg = cfg
        self.dtype = dtype
        self.device = device
        self._h = None
        L = _lib.load()
        _lib.init(device)
        if blob_device is not None:          # packed fp32 blob as a CUDA tensor (e.g. filled by an RCCL broadcast)
            import torch
            t = blob_device
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device.index == device):
                raise ValueError("blob_device must be a contiguous float32 CUDA tensor on the engine's device")
            ci = np.asarray(cfg.to_int_array(), dtype=np.int32)
            torch.cuda.current_stream(t.device).synchronize()
            self._h = L.mi_bigvgan_create_mem(_lib.i32p(ci), len(ci), t.data_ptr(), t.numel(), _lib.DTYPES[dtype], device,
                                              _lib.MI_DEVICE)
            if not self._h:
                raise _lib.MiError("mi_bigvgan_create_mem: " + L.mi_last_error().decode())
            return
        if blob is None:
            if state is None:
                raise ValueError("BigVGANVocoder needs a state dict or a packed blob")
            blob = pack_bigvgan(cfg, state)
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        ci = np.asarray(cfg.to_int_array(), dtype=np.int32)
        expect = L.mi_bigvgan_param_count(_lib.i32p(ci), len(ci))
        if expect != blob.size:
            raise _lib.MiError(f"weight blob has {blob.size} floats, config needs {expect}")
        self._h = L.mi_bigvgan_create(_lib.i32p(ci), len(ci), _lib.f32p(blob), blob.size, _lib.DTYPES[dtype], device)
        if not self._h:
            raise _lib.MiError("mi_bigvgan_create: " + L.mi_last_error().decode())

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().mi_bigvgan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def out_len(self, frames: int) -> int:
        return int(_lib.load().mi_bigvgan_out_len(self._h, frames))

    # ---- numpy in / numpy out (the reference's `.run` shape) ----------------------------------
    def run(self, mel: np.ndarray) -> np.ndarray:
        mel = self._check_mel(mel)
        B, _, F = mel.shape
        out = np.empty((B, 1, self.out_len(F)), dtype=np.int16)
        _lib.check(_lib.load().mi_bigvgan_forward(self._h, mel.ctypes.data, B, F, out.ctypes.data, _lib.MI_HOST),
                   "mi_bigvgan_forward")
        return out

    def run_float(self, mel: np.ndarray) -> np.ndarray:
        """float waveform in [-1, 1] before the int16 conversion (tests)."""
        mel = self._check_mel(mel)
        B, _, F = mel.shape
        out = np.empty((B, 1, self.out_len(F)), dtype=np.float32)
        _lib.check(_lib.load().mi_bigvgan_forward_f32(self._h, mel.ctypes.data, B, F, out.ctypes.data, _lib.MI_HOST),
                   "mi_bigvgan_forward_f32")
        return out

    # ---- torch-ROCm tensors, zero copy (device pointers cross the C-ABI) ----------------------
    def run_torch(self, mel, out=None):
        import torch
        if not (mel.is_cuda and mel.dtype == torch.float32 and mel.is_contiguous()):
            raise ValueError("mel must be a contiguous float32 tensor on the GPU")
        if mel.dim() != 3 or mel.shape[1] != self.cfg.num_mels:
            raise ValueError(f"mel must be (B, {self.cfg.num_mels}, F)")
        B, _, F = mel.shape
        if out is None:
            out = torch.empty((B, 1, self.out_len(F)), dtype=torch.int16, device=mel.device)
        torch.cuda.current_stream(mel.device).synchronize()
        _lib.check(_lib.load().mi_bigvgan_forward(self._h, mel.data_ptr(), B, F, out.data_ptr(), _lib.MI_DEVICE),
                   "mi_bigvgan_forward")
        return out

    # ---- ragged batches: items of different lengths in one forward ------------------------------------------
    def run_ragged(self, mels, return_float: bool = False):
        """mels: list of (num_mels, F_b) arrays -> list of int16 (1, 1, F_b * hop + 30), each the waveform ``run`` gives for
        that item alone (with return_float: also the float waveforms, as a second list)."""
        cfg = self.cfg
        mels = [np.asarray(m) for m in mels]
        for b, m in enumerate(mels):
            if m.ndim != 2 or m.shape[0] != cfg.num_mels:
                raise ValueError(f"item {b}: mel must be ({cfg.num_mels}, F), got {m.shape}")
        F, _, out_lens, out_offs, _ = ragged_layout(cfg, [m.shape[1] for m in mels])
        x = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(m, np.float32).reshape(-1) for m in mels]))
        n = sum(out_lens)
        out = np.empty(n, np.int16)
        outf = np.empty(n, np.float32) if return_float else None
        fr = np.asarray(F, np.int64)
        lens = np.zeros(len(F), np.int64)
        _lib.check(_lib.load().mi_bigvgan_forward_ragged(self._h, len(F), x.ctypes.data, fr.ctypes.data, out.ctypes.data,
                                                         None if outf is None else outf.ctypes.data, n, lens.ctypes.data,
                                                         _lib.MI_HOST), "mi_bigvgan_forward_ragged")
        assert list(lens) == out_lens, (list(lens), out_lens)
        wav = [out[o:o + l].reshape(1, 1, l).copy() for o, l in zip(out_offs, out_lens)]
        if return_float:
            return wav, [outf[o:o + l].reshape(1, 1, l).copy() for o, l in zip(out_offs, out_lens)]
        return wav

    def run_ragged_torch(self, mel_cat, frames, out=None):
        """Device-resident run_ragged: mel_cat = the items' (num_mels, F_b) mels concatenated (float32 CUDA tensor, e.g. from
        ``F5Engine.synthesize_mel_ragged_torch``), frames = the host list F_b.  Returns (wav_cat, out_lens): the int16 waveforms
        concatenated in one CUDA tensor and their lengths."""
        import torch
        cfg = self.cfg
        F, _, out_lens, _, _ = ragged_layout(cfg, frames)
        if not (mel_cat.is_cuda and mel_cat.dtype == torch.float32 and mel_cat.is_contiguous()):
            raise ValueError("mel_cat must be a contiguous float32 tensor on the GPU")
        if mel_cat.numel() < sum(F) * cfg.num_mels:
            raise ValueError("mel_cat holds fewer than sum(frames) * num_mels values")
        n = sum(out_lens)
        if out is None:
            out = torch.empty(n, dtype=torch.int16, device=mel_cat.device)
        assert out.is_cuda and out.dtype == torch.int16 and out.is_contiguous()
        fr = np.asarray(F, np.int64)
        lens = np.zeros(len(F), np.int64)
        torch.cuda.current_stream(mel_cat.device).synchronize()
        _lib.check(_lib.load().mi_bigvgan_forward_ragged(self._h, len(F), mel_cat.data_ptr(), fr.ctypes.data, out.data_ptr(), None,
                                                         out.numel(), lens.ctypes.data, _lib.MI_DEVICE), "mi_bigvgan_forward_ragged")
        return out, [int(v) for v in lens]

    def run_latent_ragged(self, latents, conds, return_float: bool = False):
        """IndexTTS graph F for B sentences of one speaker: latents = list of (T_b >= 3, gpt_dim) arrays, conds as in
        ``run_latent`` (shared by all items) -> list of int16 (1, 1, (T_b - 2) * hop + 30).  The one-voice form of
        ``run_latent_voices``."""
        cfg = self.cfg
        if not (cfg.pre_layernorm and cfg.speaker_cond):
            raise ValueError("this vocoder was not created from an IndexTTS graph-F config")
        latents = [np.asarray(x) for x in latents]
        for b, x in enumerate(latents):
            if x.ndim != 2 or x.shape[1] != cfg.num_mels:
                raise ValueError(f"item {b}: latent must be (T_codes, {cfg.num_mels}), got {x.shape}")
        _, _, out_lens, out_offs, _ = ragged_layout(cfg, [x.shape[0] for x in latents], latent=True)
        flat = self._flat_conds(conds)
        x = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(v, np.float32) for v in latents]))
        tc = np.asarray([v.shape[0] for v in latents], np.int64)
        n = sum(out_lens)
        out = np.empty(n, np.int16)
        outf = np.empty(n, np.float32) if return_float else None
        lens = np.zeros(len(latents), np.int64)
        _lib.check(_lib.load().mi_bigvgan_forward_latent_ragged(self._h, len(latents), x.ctypes.data, tc.ctypes.data, flat.ctypes.data,
                                                                flat.size, out.ctypes.data, None if outf is None else outf.ctypes.data,
                                                                n, lens.ctypes.data, _lib.MI_HOST), "mi_bigvgan_forward_latent_ragged")
        assert list(lens) == out_lens, (list(lens), out_lens)
        wav = [out[o:o + l].reshape(1, 1, l).copy() for o, l in zip(out_offs, out_lens)]
        if return_float:
            return wav, [outf[o:o + l].reshape(1, 1, l).copy() for o, l in zip(out_offs, out_lens)]
        return wav

    def run_latent_voices(self, latents, voices, voice_of, return_float: bool = False):
        """IndexTTS graph F for B sentences of several speakers in one forward: latents as in ``run_latent_ragged``, voices = list
        of V conditioning lists as ``run_latent`` takes them, voice_of[b] = the voice of sentence b.  Returns what
        ``run_latent_ragged`` returns; item b is the waveform ``run_latent(latents[b], voices[voice_of[b]])`` gives."""
        cfg = self.cfg
        if not (cfg.pre_layernorm and cfg.speaker_cond):
            raise ValueError("this vocoder was not created from an IndexTTS graph-F config")
        latents = [np.asarray(x) for x in latents]
        for b, x in enumerate(latents):
            if x.ndim != 2 or x.shape[1] != cfg.num_mels:
                raise ValueError(f"item {b}: latent must be (T_codes, {cfg.num_mels}), got {x.shape}")
        _, _, out_lens, out_offs, _ = ragged_layout(cfg, [x.shape[0] for x in latents], latent=True)
        table, index = voices_table(cfg, voices, voice_of, len(latents))
        x = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(v, np.float32) for v in latents]))
        tc = np.asarray([v.shape[0] for v in latents], np.int64)
        n = sum(out_lens)
        out = np.empty(n, np.int16)
        outf = np.empty(n, np.float32) if return_float else None
        lens = np.zeros(len(latents), np.int64)
        _lib.check(_lib.load().mi_bigvgan_forward_latent_voices(self._h, len(latents), x.ctypes.data, tc.ctypes.data, table.shape[0],
                                                                table.ctypes.data, table.shape[1], index.ctypes.data, out.ctypes.data,
                                                                None if outf is None else outf.ctypes.data, n, lens.ctypes.data,
                                                                _lib.MI_HOST), "mi_bigvgan_forward_latent_voices")
        assert list(lens) == out_lens, (list(lens), out_lens)
        wav = [out[o:o + l].reshape(1, 1, l).copy() for o, l in zip(out_offs, out_lens)]
        if return_float:
            return wav, [outf[o:o + l].reshape(1, 1, l).copy() for o, l in zip(out_offs, out_lens)]
        return wav

    def run_latent_voices_torch(self, latent_cat, t_codes, conds_table, voice_of, out=None):
        """Device-resident run_latent_voices: latent_cat = the items' (T_b, gpt_dim) latents concatenated (float32 CUDA tensor, e.g.
        the hidden states a GPT queue left on the device), t_codes = the host list T_b, conds_table = (V, total_cond) float32 CUDA
        tensor (rows as ``flat_conds``), voice_of = the host list of voice indices.  The conditioning is read where it lies.
        Returns (wav_cat, out_lens): the int16 waveforms concatenated in one CUDA tensor and their lengths."""
        import torch
        cfg = self.cfg
        if not (cfg.pre_layernorm and cfg.speaker_cond):
            raise ValueError("this vocoder was not created from an IndexTTS graph-F config")
        _, _, out_lens, _, _ = ragged_layout(cfg, t_codes, latent=True)
        tc = np.asarray([int(t) for t in t_codes], np.int64)
        if not (latent_cat.is_cuda and latent_cat.dtype == torch.float32 and latent_cat.is_contiguous()):
            raise ValueError("latent_cat must be a contiguous float32 tensor on the GPU")
        if latent_cat.numel() < int(tc.sum()) * cfg.num_mels:
            raise ValueError("latent_cat holds fewer than sum(t_codes) * gpt_dim values")
        if not (conds_table.is_cuda and conds_table.dtype == torch.float32 and conds_table.is_contiguous() and conds_table.dim() == 2):
            raise ValueError("conds_table must be a contiguous float32 (V, total_cond) tensor on the GPU")
        want = sum(cfg.stage_channels(i) for i in range(cfg.num_upsamples)) + cfg.upsample_initial_channel
        V = int(conds_table.shape[0])
        if V < 1 or int(conds_table.shape[1]) != want:
            raise ValueError(f"conds_table must be (V >= 1, {want}), got {tuple(conds_table.shape)}")
        try:
            index = [operator.index(x) for x in voice_of]
        except TypeError:
            raise ValueError("voice_of must hold integers") from None
        if len(index) != len(tc) or any(not 0 <= x < V for x in index):
            raise ValueError(f"voice_of must hold {len(tc)} indices in [0, {V})")
        index = np.asarray(index, np.int32)
        n = sum(out_lens)
        if out is None:
            out = torch.empty(n, dtype=torch.int16, device=latent_cat.device)
        assert out.is_cuda and out.dtype == torch.int16 and out.is_contiguous()
        lens = np.zeros(len(tc), np.int64)
        torch.cuda.current_stream(latent_cat.device).synchronize()
        _lib.check(_lib.load().mi_bigvgan_forward_latent_voices(self._h, len(tc), latent_cat.data_ptr(), tc.ctypes.data, V,
                                                                conds_table.data_ptr(), want, index.ctypes.data, out.data_ptr(), None,
                                                                out.numel(), lens.ctypes.data, _lib.MI_DEVICE),
                   "mi_bigvgan_forward_latent_voices")
        return out, [int(v) for v in lens]

    # ---- windows of latent rows with halo frames: audio before a sentence has all its rows ------------------------------------
    def run_latent_windows(self, latent, windows, voices, voice_of, return_float: bool = False):
        """IndexTTS graph F on windows of one latent array: latent (latent_rows, gpt_dim) float32 (no rows are dropped here: leave
        a sentence's last two rows out of its windows), windows = (row0, rows, head, tail) each (``window_layout``), voices /
        voice_of as in ``run_latent_voices`` with one entry of voice_of per window.  Returns a list of int16 (out_len,) arrays,
        the kept samples of each window (with return_float: also the float samples, as a second list).  With halo >=
        ``cfg.halo_frames()`` at every cut inside a sentence the pieces are the sentence's own samples."""
        cfg = self.cfg
        latent = np.ascontiguousarray(latent, dtype=np.float32)
        if latent.ndim != 2 or latent.shape[1] != cfg.num_mels:
            raise ValueError(f"latent must be (latent_rows, {cfg.num_mels}), got {latent.shape}")
        win = [tuple(int(v) for v in w) for w in windows]
        _, out_lens, out_offs, _ = window_layout(cfg, latent.shape[0], win)
        table, index = voices_table(cfg, voices, voice_of, len(win))
        n = sum(out_lens)
        out = np.empty(n, np.int16)
        outf = np.empty(n, np.float32) if return_float else None
        lens = np.zeros(len(win), np.int64)
        w = np.asarray(win, np.int64)
        row0, rows = np.ascontiguousarray(w[:, 0]), np.ascontiguousarray(w[:, 1])
        head, tail = np.ascontiguousarray(w[:, 2], np.int32), np.ascontiguousarray(w[:, 3], np.int32)
        _lib.check(_lib.load().mi_bigvgan_forward_latent_windows(self._h, len(win), latent.ctypes.data, latent.shape[0], row0.ctypes.data,
                                                                 rows.ctypes.data, head.ctypes.data, tail.ctypes.data, table.shape[0],
                                                                 table.ctypes.data, table.shape[1], index.ctypes.data, out.ctypes.data,
                                                                 None if outf is None else outf.ctypes.data, n, lens.ctypes.data,
                                                                 _lib.MI_HOST), "mi_bigvgan_forward_latent_windows")
        assert list(lens) == out_lens, (list(lens), out_lens)
        wav = [out[o:o + l].copy() for o, l in zip(out_offs, out_lens)]
        if return_float:
            return wav, [outf[o:o + l].copy() for o, l in zip(out_offs, out_lens)]
        return wav

    def run_latent_windows_torch(self, latent, windows, conds_table, voice_of, out=None, out_float=None):
        """Device-resident run_latent_windows: latent = a contiguous float32 CUDA tensor whose last dimension is gpt_dim, read as
        (latent_rows, gpt_dim) rows where it lies (e.g. the (n, cap, hidden) `hidden` tensor of an IndexGPT queue session:
        sentence i's rows start at i * cap); conds_table / voice_of as in ``run_latent_voices_torch``.  `out` (int16) may be
        larger than the kept samples; nothing outside them is written.  out_float: an optional float32 tensor for the float
        samples.  Returns (wav_cat, out_lens)."""
        import torch
        cfg = self.cfg
        if not (latent.is_cuda and latent.dtype == torch.float32 and latent.is_contiguous() and latent.dim() >= 2
                and latent.shape[-1] == cfg.num_mels):
            raise ValueError(f"latent must be a contiguous float32 (..., {cfg.num_mels}) tensor on the GPU")
        n_rows = latent.numel() // cfg.num_mels
        win = [tuple(int(v) for v in w) for w in windows]
        _, out_lens, _, _ = window_layout(cfg, n_rows, win)
        if not (conds_table.is_cuda and conds_table.dtype == torch.float32 and conds_table.is_contiguous() and conds_table.dim() == 2):
            raise ValueError("conds_table must be a contiguous float32 (V, total_cond) tensor on the GPU")
        want = sum(cfg.stage_channels(i) for i in range(cfg.num_upsamples)) + cfg.upsample_initial_channel
        V = int(conds_table.shape[0])
        if V < 1 or int(conds_table.shape[1]) != want:
            raise ValueError(f"conds_table must be (V >= 1, {want}), got {tuple(conds_table.shape)}")
        try:
            index = [operator.index(x) for x in voice_of]
        except TypeError:
            raise ValueError("voice_of must hold integers") from None
        if len(index) != len(win) or any(not 0 <= x < V for x in index):
            raise ValueError(f"voice_of must hold {len(win)} indices in [0, {V})")
        index = np.asarray(index, np.int32)
        n = sum(out_lens)
        if out is None:
            out = torch.empty(n, dtype=torch.int16, device=latent.device)
        if not (out.is_cuda and out.dtype == torch.int16 and out.is_contiguous() and out.numel() >= n):
            raise ValueError(f"out must be a contiguous int16 CUDA tensor of at least {n} samples")
        cap = out.numel()
        if out_float is not None:
            if not (out_float.is_cuda and out_float.dtype == torch.float32 and out_float.is_contiguous() and out_float.numel() >= n):
                raise ValueError(f"out_float must be a contiguous float32 CUDA tensor of at least {n} samples")
            cap = min(cap, out_float.numel())
        lens = np.zeros(len(win), np.int64)
        w = np.asarray(win, np.int64)
        row0, rows = np.ascontiguousarray(w[:, 0]), np.ascontiguousarray(w[:, 1])
        head, tail = np.ascontiguousarray(w[:, 2], np.int32), np.ascontiguousarray(w[:, 3], np.int32)
        torch.cuda.current_stream(latent.device).synchronize()
        _lib.check(_lib.load().mi_bigvgan_forward_latent_windows(self._h, len(win), latent.data_ptr(), n_rows, row0.ctypes.data,
                                                                 rows.ctypes.data, head.ctypes.data, tail.ctypes.data, V,
                                                                 conds_table.data_ptr(), want, index.ctypes.data, out.data_ptr(),
                                                                 None if out_float is None else out_float.data_ptr(), cap,
                                                                 lens.ctypes.data, _lib.MI_DEVICE), "mi_bigvgan_forward_latent_windows")
        return out, [int(v) for v in lens]

    def _flat_conds(self, conds):
        return flat_conds(self.cfg, conds)

    # ---- IndexTTS graph F: latent + speaker conditioning in, waveform out ------------------------------------
    def run_latent(self, latent: np.ndarray, conds, return_float: bool = False):
        """latent (T_codes, gpt_dim) float32 ('save_hidden_state'); conds = [save_bigvgan_conds_0..n-1,
        bigvgan_cond_layer_speaker_embedding], each (1, C, 1) / (C,).  Returns int16 (1, 1, (T_codes-2)*hop + 30)."""
        cfg = self.cfg
        if not (cfg.pre_layernorm and cfg.speaker_cond):
            raise ValueError("this vocoder was not created from an IndexTTS graph-F config")
        latent = np.ascontiguousarray(latent, dtype=np.float32)
        if latent.ndim != 2 or latent.shape[1] != cfg.num_mels or latent.shape[0] < 3:
            raise ValueError(f"save_hidden_state must be (T_codes >= 3, {cfg.num_mels}), got {latent.shape}")
        flat = self._flat_conds(conds)
        T = latent.shape[0]
        n = (T - 2) * cfg.hop + 30
        out = np.empty((1, 1, n), np.int16)
        outf = np.empty((1, 1, n), np.float32) if return_float else None
        _lib.check(_lib.load().mi_bigvgan_forward_latent(self._h, latent.ctypes.data, T, flat.ctypes.data, flat.size,
                                                         out.ctypes.data, None if outf is None else outf.ctypes.data,
                                                         _lib.MI_HOST), "mi_bigvgan_forward_latent")
        return (out, outf) if return_float else out

    def run_latent_torch(self, latent, conds_flat, out=None):
        """Device-resident variant: latent (T_codes, gpt_dim) float32 CUDA tensor, conds_flat = the concatenated
        conditioning vectors (float32 CUDA tensor, total_cond values)."""
        import torch
        cfg = self.cfg
        assert latent.is_cuda and latent.dtype == torch.float32 and latent.is_contiguous()
        assert conds_flat.is_cuda and conds_flat.dtype == torch.float32 and conds_flat.is_contiguous()
        T = latent.shape[0]
        if out is None:
            out = torch.empty((1, 1, (T - 2) * cfg.hop + 30), dtype=torch.int16, device=latent.device)
        torch.cuda.current_stream(latent.device).synchronize()
        _lib.check(_lib.load().mi_bigvgan_forward_latent(self._h, latent.data_ptr(), T, conds_flat.data_ptr(),
                                                         conds_flat.numel(), out.data_ptr(), None, _lib.MI_DEVICE),
                   "mi_bigvgan_forward_latent")
        return out

    def _check_mel(self, mel):
        mel = np.asarray(mel)
        if mel.ndim != 3 or mel.shape[1] != self.cfg.num_mels or mel.shape[2] < 1 or mel.shape[0] < 1:
            raise ValueError(f"mel_features must be (B, {self.cfg.num_mels}, F>=1), got {mel.shape}")
        if mel.dtype == np.float16:
            mel = mel.astype(np.float32)
        if mel.dtype != np.float32:
            raise ValueError(f"mel_features must be float32/float16, got {mel.dtype}")
        return np.ascontiguousarray(mel)


# ---- unit-level ops (tests) --------------------------------------------------------------------
def aa_activation1d(x, alpha_log, beta_log, *, post=False, logscale=True, dtype="f32"):
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, Cc, T = x.shape
    a = np.ascontiguousarray(alpha_log, dtype=np.float32)
    b = np.ascontiguousarray(beta_log, dtype=np.float32)
    y = np.empty((B, Cc, T + (30 if post else 0)), dtype=np.float32)
    _lib.check(_lib.load().mi_aa_activation1d(_lib.f32p(x), B, Cc, T, _lib.f32p(a), _lib.f32p(b), int(logscale),
                                              int(post), _lib.DTYPES[dtype], _lib.f32p(y)), "mi_aa_activation1d")
    return y


def aa_conv1d(x, alpha_log, beta_log, w, b, *, dilation=1, res=None, logscale=True, dtype="f32"):
    """The fused kernel of the low-channel stages: conv(Activation1d(x)) (+ res), "same" padding; C % 8 == 0, C <= 96."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    w = np.ascontiguousarray(w, dtype=np.float32)
    B, Cc, T = x.shape
    if w.shape[0] != Cc or w.shape[1] != Cc:
        raise ValueError("aa_conv1d: weight must be (C, C, k)")
    a = np.ascontiguousarray(alpha_log, dtype=np.float32)
    bb = np.ascontiguousarray(beta_log, dtype=np.float32)
    bias = np.ascontiguousarray(b, dtype=np.float32)
    r = np.ascontiguousarray(res, dtype=np.float32) if res is not None else None
    y = np.empty_like(x)
    _lib.check(_lib.load().mi_aa_conv1d(_lib.f32p(x), B, Cc, T, _lib.f32p(a), _lib.f32p(bb), int(logscale), _lib.f32p(w),
                                        _lib.f32p(bias), w.shape[2], dilation, _lib.f32p(r) if r is not None else None,
                                        _lib.DTYPES[dtype], _lib.f32p(y)), "mi_aa_conv1d")
    return y


def conv1d(x, w, b=None, *, dilation=1, padding=0, groups=1, dtype="f32"):
    x = np.ascontiguousarray(x, dtype=np.float32)
    w = np.ascontiguousarray(w, dtype=np.float32)
    B, Ci, T = x.shape
    Co, _, k = w.shape
    To = T + 2 * padding - dilation * (k - 1)
    y = np.empty((B, Co, To), dtype=np.float32)
    bp = _lib.f32p(np.ascontiguousarray(b, dtype=np.float32)) if b is not None else None
    _lib.check(_lib.load().mi_conv1d(_lib.f32p(x), B, Ci, T, _lib.f32p(w), bp, Co, k, dilation, padding, groups,
                                     _lib.DTYPES[dtype], _lib.f32p(y)), "mi_conv1d")
    return y


def conv_transpose1d(x, w, b=None, *, stride, padding, dtype="f32"):
    x = np.ascontiguousarray(x, dtype=np.float32)
    w = np.ascontiguousarray(w, dtype=np.float32)
    B, Ci, T = x.shape
    _, Co, k = w.shape
    y = np.empty((B, Co, (T - 1) * stride - 2 * padding + k), dtype=np.float32)
    bp = _lib.f32p(np.ascontiguousarray(b, dtype=np.float32)) if b is not None else None
    _lib.check(_lib.load().mi_conv_transpose1d(_lib.f32p(x), B, Ci, T, _lib.f32p(w), bp, Co, k, stride, padding,
                                               _lib.DTYPES[dtype], _lib.f32p(y)), "mi_conv_transpose1d")
    return y
