#!/usr/bin/env python3
"""Timing of ragged BigVGAN batches (mi_bigvgan_forward_ragged / mi_bigvgan_forward_latent_ragged) against the same items run
alone and against a uniform batch at (B, Fmax).

    python tools/bigvgan_ragged_bench.py [--reps 7] [--frames 512,470,390,300,256,200,150,97] [--codes 256,...]

Two workloads, full-size weights, in one process; the three runs alternate inside every repetition and the median is reported:
  mel vocoder (fp16 by default, device-resident tensors):
    (a) ragged: the B mels in one call (run_ragged_torch);
    (b) alone: the same mels one call each (run_torch, summed);
    (c) uniform: one (B, 100, Fmax) batch (run_torch).
  graph F (IndexTTS, fp16, host arrays as IndexTTS hands them over): 16 sentences of 97-256 codes by default;
    (a) ragged (run_latent_ragged); (b) alone (run_latent per sentence, summed); (c) full length: the ragged entry with every
    sentence at the longest length.  Graph F has no batched uniform entry, so (c) is NOT a uniform run: it is the same
    length-aware kernels with every row live, and (a) / (c) measures what the dead tiles save.
Prints one JSON line per workload: ms per call, live frames / (B * Fmax), and ragged over the other two.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "text-to-speech-tts-onnx_amd"))

import numpy as np  # noqa: E402

from mi355tts import weights as W  # noqa: E402
from mi355tts.bigvgan import BigVGANVocoder  # noqa: E402
from mi355tts.config import BigVGANConfig  # noqa: E402


def alternating(fns, reps, sync):
    for f in fns:                                  # warm-up: workspace, side streams, code objects
        f(); f()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            sync(); t0 = time.perf_counter(); f(); sync(); ts[i].append(time.perf_counter() - t0)
    return [float(np.median(t)) * 1e3 for t in ts]


def report(name, frames, ta, tb, tc, third, extra):
    Fmax = max(frames)
    res = {"workload": name, **extra, "frames": frames, "live_fraction": round(sum(frames) / (len(frames) * Fmax), 3),
           "ragged_ms": round(ta, 2), "alone_ms": round(tb, 2), f"{third}_ms": round(tc, 2),
           f"ragged_over_{third}": round(ta / tc, 3), "ragged_over_alone": round(ta / tb, 3)}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--frames", default="512,470,390,300,256,200,150,97")
    ap.add_argument("--codes", default="")
    ap.add_argument("--skip-graph-f", action="store_true")
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize

    cfg = BigVGANConfig()
    v = BigVGANVocoder(cfg, W.synth_state(W.bigvgan_spec(cfg), 9527), dtype=a.dtype)
    frames = [int(x) for x in a.frames.split(",")]
    B, Fmax = len(frames), max(frames)
    mel8 = W.bigvgan_synthetic_mel(cfg, B, Fmax, 0)
    mels = [torch.from_numpy(np.ascontiguousarray(mel8[b][:, :f])).to(dev) for b, f in enumerate(frames)]
    mel_cat = torch.cat([m.reshape(-1) for m in mels])
    alone_in = [m[None].contiguous() for m in mels]
    uni = torch.from_numpy(np.ascontiguousarray(mel8)).to(dev)
    ta, tb, tc = alternating([lambda: v.run_ragged_torch(mel_cat, frames),
                              lambda: [v.run_torch(m) for m in alone_in],
                              lambda: v.run_torch(uni)], a.reps, sync)
    v.close()
    report("bigvgan_mel", frames, ta, tb, tc, "uniform", {"dtype": a.dtype})

    if a.skip_graph_f:
        return
    gcfg = BigVGANConfig.indextts()
    g = BigVGANVocoder(gcfg, W.synth_state(W.bigvgan_spec(gcfg), 9527), dtype=a.dtype)
    codes = [int(x) for x in a.codes.split(",")] if a.codes else [int(c) for c in np.linspace(97, 256, 16).round()]
    lat = [W.synth_normal(100 + i, "latent", (c, gcfg.num_mels)) for i, c in enumerate(codes)]
    want = [gcfg.stage_channels(i) for i in range(gcfg.num_upsamples)] + [gcfg.upsample_initial_channel]
    conds = [W.synth_normal(200 + i, "cond", (n,), std=0.1) for i, n in enumerate(want)]
    Tmax = max(codes)
    lat_max = [W.synth_normal(100 + i, "latent", (Tmax, gcfg.num_mels)) for i in range(len(codes))]
    ta, tb, tc = alternating([lambda: g.run_latent_ragged(lat, conds),
                              lambda: [g.run_latent(x, conds) for x in lat],
                              lambda: g.run_latent_ragged(lat_max, conds)], a.reps, sync)
    g.close()
    report("indextts_graph_f", [c - 2 for c in codes], ta, tb, tc, "full_length", {"dtype": a.dtype, "codes": codes})


if __name__ == "__main__":
    main()
