#!/usr/bin/env python3
"""Timing of a ragged F5 batch (mi_f5_synthesize_ragged) against the same utterances run alone and against a uniform batch.

    python tools/f5_ragged_bench.py [--dtypes f32,bf16] [--reps 3] [--lengths 700,900,1126,1268]

For each engine dtype, end to end (front end + 31 evaluations on a replayed hipGraph + Vocos), per call after two warm-up calls:
  (a) ragged: the U utterances of max_duration N_u in one call;
  (b) alone: the same utterances one after the other (one call each);
  (c) uniform: a U-utterance batch at N = max N_u (mi_f5_synthesize).
Prints ms per call, ms per sampling step (call / (nfe - 1)) and audio seconds generated per second, one JSON line per dtype.
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
from mi355tts.config import F5Config  # noqa: E402
from mi355tts.f5 import F5Engine  # noqa: E402


def timed(fn, reps):
    fn(); fn()                                     # eager, then the graph capture
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lengths", default="700,900,1126,1268")
    a = ap.parse_args()
    cfg = F5Config()
    Ns = [int(x) for x in a.lengths.split(",")]
    U = len(Ns)
    raw = W.synth_state(W.f5_spec(cfg), 9527)
    audio, ids, _, _ = W.f5_synthetic_inputs(cfg, U, 0)
    noise = [W.synth_normal(9527 + u, "noise", (n, cfg.mel_dim)) for u, n in enumerate(Ns)]
    Nmax = max(Ns)
    uni_noise = np.stack([W.synth_normal(9527 + u, "noise", (Nmax, cfg.mel_dim)) for u in range(U)])
    R = cfg.ref_frames(audio.shape[1])
    steps = cfg.nfe_step - 1
    sec = lambda ns: sum((n - R - 1) * cfg.hop_length for n in ns) / cfg.sample_rate
    for dt in a.dtypes.split(","):
        eng = F5Engine(cfg, raw, dtype=dt)
        ta = timed(lambda: eng.synthesize_ragged(list(audio), list(ids), Ns, noise=noise), a.reps)
        tb = sum(timed(lambda u=u: eng.synthesize(audio[u:u + 1], ids[u:u + 1], Ns[u], noise=noise[u][None]), a.reps) for u in range(U))
        tc = timed(lambda: eng.synthesize(audio, ids, Nmax, noise=uni_noise), a.reps)
        eng.close()
        res = {"dtype": dt, "lengths": Ns}
        for k, t, ns in (("ragged", ta, Ns), ("alone", tb, Ns), ("uniform", tc, [Nmax] * U)):
            res[k] = {"ms": round(t * 1e3, 1), "ms_per_step": round(t * 1e3 / steps, 2), "audio_s_per_s": round(sec(ns) / t, 2)}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
