#!/usr/bin/env python3
"""Timing of the several-voice graph-F forward (mi_bigvgan_forward_latent_voices) against what a caller had to do before it:
sort the finished sentences by voice and run one ragged forward per voice.

    python tools/indextts_voices_bench.py [--voices 1,2,4,16] [--sentences 16] [--lo 60] [--hi 240] [--seed 0] [--dtype f16]
                                          [--forms host,torch] [--build NAME]

Full IndexTTS graph-F size, synthetic weights.  The sentences' code counts are seeded-uniform in [lo, hi] (the range of
tools/gpt_queue_bench.py); V voices are assigned round-robin (sentence i speaks with voice i mod V).  Per V and per form
(host: numpy arrays through MI_HOST; torch: latents, conditioning and waveforms stay on the device) it times
  (a) one run_latent_voices call over all sentences;
  (b) V calls of the one-voice ragged forward, one per voice, on that voice's sentences
as synchronised wall clock: the median of three calls after one warm call, with the spread (max - min) / median.  One JSON line per
configuration carrying `build` and `tool`; `a_beats_b` only when the difference exceeds three times the larger spread.

A library without the new entry (an older build loaded through MI355TTS_LIB) is timed on (b) alone: at V = 1 that is the one-voice
ragged forward, the yardstick for the rerouted path.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "text-to-speech-tts-onnx_amd"))

import numpy as np  # noqa: E402

from mi355tts import _lib  # noqa: E402
from mi355tts import weights as W  # noqa: E402
from mi355tts.bigvgan import BigVGANVocoder, flat_conds  # noqa: E402
from mi355tts.config import BigVGANConfig  # noqa: E402


def timed(fn, sync):
    fn(); sync()                                   # warm: workspace, side streams, code objects
    ts = []
    for _ in range(3):
        sync(); t0 = time.perf_counter(); fn(); sync(); ts.append(time.perf_counter() - t0)
    med = float(np.median(ts))
    return med * 1e3, (max(ts) - min(ts)) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voices", default="1,2,4,16")
    ap.add_argument("--sentences", type=int, default=16)
    ap.add_argument("--lo", type=int, default=60)
    ap.add_argument("--hi", type=int, default=240)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--forms", default="host,torch")
    ap.add_argument("--build", default="", help="label of the library under test (default: its file name)")
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    L = _lib.load()
    has_voices = hasattr(L, "mi_bigvgan_forward_latent_voices")
    build = a.build or os.path.basename(_lib.lib_path())

    cfg = BigVGANConfig.indextts()
    v = BigVGANVocoder(cfg, W.synth_state(W.bigvgan_spec(cfg), 9527), dtype=a.dtype)
    n = a.sentences
    codes = [int(c) for c in np.random.default_rng(a.seed).integers(a.lo, a.hi + 1, n)]
    lats = [W.synth_normal(100 + i, "lat", (c, cfg.num_mels), std=1.0) for i, c in enumerate(codes)]
    sizes = [cfg.stage_channels(i) for i in range(cfg.num_upsamples)] + [cfg.upsample_initial_channel]
    vmax = max(int(x) for x in a.voices.split(","))
    voices = [[W.synth_normal(1000 * (k + 1) + i, "cond", (m,), std=0.2) for i, m in enumerate(sizes)] for k in range(vmax)]
    flat = [flat_conds(cfg, c) for c in voices]
    hop = cfg.hop

    def ragged_device(lat_cat, tcs, cond_row, out):
        """the one-voice ragged entry on device pointers (there in every build)"""
        tc = np.asarray(tcs, np.int64)
        lens = np.zeros(len(tcs), np.int64)
        _lib.check(L.mi_bigvgan_forward_latent_ragged(v._h, len(tcs), lat_cat.data_ptr(), tc.ctypes.data, cond_row.data_ptr(),
                                                      cond_row.numel(), out.data_ptr(), None, out.numel(), lens.ctypes.data,
                                                      _lib.MI_DEVICE), "mi_bigvgan_forward_latent_ragged")

    for V in [int(x) for x in a.voices.split(",")]:
        voice_of = [i % V for i in range(n)]
        groups = [[i for i in range(n) if voice_of[i] == k] for k in range(V)]
        groups = [g for g in groups if g]
        for form in a.forms.split(","):
            if form == "host":
                def run_a():
                    v.run_latent_voices(lats, voices[:V], voice_of)

                def run_b():
                    for g in groups:
                        v.run_latent_ragged([lats[i] for i in g], voices[voice_of[g[0]]])
            else:
                lat_cat = torch.from_numpy(np.ascontiguousarray(np.concatenate(lats))).to(dev)
                tab = torch.from_numpy(np.ascontiguousarray(np.stack(flat[:V]))).to(dev)
                out = torch.empty(sum((c - 2) * hop + 30 for c in codes), dtype=torch.int16, device=dev)
                g_lat = [torch.from_numpy(np.ascontiguousarray(np.concatenate([lats[i] for i in g]))).to(dev) for g in groups]
                g_tc = [[codes[i] for i in g] for g in groups]
                g_out = [torch.empty(sum((c - 2) * hop + 30 for c in t), dtype=torch.int16, device=dev) for t in g_tc]

                def run_a():
                    v.run_latent_voices_torch(lat_cat, codes, tab, voice_of, out=out)

                def run_b():
                    for k, g in enumerate(groups):
                        ragged_device(g_lat[k], g_tc[k], tab[voice_of[g[0]]], g_out[k])
            res = {"tool": "indextts_voices_bench", "build": build, "dtype": a.dtype, "form": form, "voices": V, "sentences": n,
                   "codes": int(sum(codes)), "codes_min": min(codes), "codes_max": max(codes)}
            tb, sb = timed(run_b, sync)
            res.update(b_per_voice_ms=round(tb, 3), b_spread=round(sb, 4), b_calls=len(groups))
            if has_voices:
                ta, sa = timed(run_a, sync)
                res.update(a_one_call_ms=round(ta, 3), a_spread=round(sa, 4), a_over_b=round(ta / tb, 4),
                           spread_max=round(max(sa, sb), 4), a_beats_b=bool(tb - ta > 3 * max(sa * ta, sb * tb)),
                           differ=bool(abs(tb - ta) > 3 * max(sa * ta, sb * tb)))
            print(json.dumps(res), flush=True)
    v.close()


if __name__ == "__main__":
    main()
