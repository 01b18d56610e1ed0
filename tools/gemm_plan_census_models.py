#!/usr/bin/env python
"""The label census of tools/gemm_plan_census.py for whole models: one evaluation each of F5 (f32 / bf16 / f16, 1 and 8 utterances
of 1126 frames), BigVGAN f16 (B = 1; B = 8 ragged) and the IndexTTS conditioning graph, synthetic weights, with the library
profiler on.  One JSON line per (model, kernel label) with its launch count, and per model the SHA-256 of its outputs: two builds
that launch the same and compute the same write the same file.

    python tools/gemm_plan_census_models.py OUT.jsonl [f5] [bigvgan] [cond]
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "text-to-speech-tts-onnx_amd")]
import numpy as np
from mi355tts import _lib, weights as W
from mi355tts.config import F5Config, BigVGANConfig, IndexCondConfig
out = open(sys.argv[1], "w")
which = sys.argv[2:] or ["f5", "bigvgan", "cond"]

def sha(*arrs):
    h = hashlib.sha256()
    for a in arrs:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()

def record(name, fn):
    fn()                                  # warm (load-time tables, workspaces)
    _lib.prof_enable(True); _lib.prof_reset()
    res = fn()
    ks = sorted(_lib.prof_kernels(), key=lambda k: k["kernel"])
    _lib.prof_enable(())
    for k in ks:
        out.write(json.dumps({"model": name, "kernel": k["kernel"], "family": k["family"], "launches": k["launches"]}) + "\n")
    out.write(json.dumps({"model": name, "sha256": sha(*res)}) + "\n")
    out.flush()
    print(name, len(ks), "labels", flush=True)

_lib.init(0)
if "f5" in which:
    from mi355tts.f5 import F5Engine
    cfg = F5Config(); N = 1126
    st = W.synth_state(W.f5_spec(cfg), 9527, fast=True)
    for dt in ("f32", "bf16", "f16"):
        eng = F5Engine(cfg, st, dtype=dt)
        for U in (1, 8):
            noise = np.stack([W.synth_normal_fast(1 + u, "n", (N, cfg.mel_dim)) for u in range(U)])
            cmt = np.stack([W.synth_normal_fast(20 + u, "c", (N, cfg.mel_dim + cfg.text_dim), std=0.7) for u in range(U)])
            cmtd = np.stack([W.synth_normal_fast(40 + u, "d", (N, cfg.mel_dim + cfg.text_dim), std=0.7) for u in range(U)])
            record(f"f5 {dt} U={U}", lambda: [np.asarray(eng.dit_eval(noise, cmt, cmtd, 3))])
        eng.close()
if "bigvgan" in which:
    from mi355tts.bigvgan import BigVGANVocoder
    cfg = BigVGANConfig()
    voc = BigVGANVocoder(cfg, W.synth_state(W.bigvgan_spec(cfg), 9527, fast=True), dtype="f16")
    mel1 = W.bigvgan_synthetic_mel(cfg, 1, 512, 0)
    record("bigvgan f16 B=1", lambda: [voc.run(mel1)])
    mel8 = W.bigvgan_synthetic_mel(cfg, 8, 512, 0)
    mels = [mel8[b, :, :512 - 37 * b] for b in range(8)]
    record("bigvgan f16 B=8 ragged", lambda: list(voc.run_ragged(mels)))
    voc.close()
if "cond" in which:
    from mi355tts.indextts import IndexCond
    cfg = IndexCondConfig()
    eng = IndexCond(cfg, W.synth_state(W.cond_spec(cfg), 9527, fast=True))
    rng = np.random.default_rng(5)
    t = np.arange(48000) / 24000.0
    audio = np.clip(0.25 * 32767 * np.sin(2 * np.pi * 140.0 * t) * (1 + 0.4 * np.sin(2 * np.pi * 2.0 * t)) + rng.normal(0, 800, t.size), -32768, 32767).astype(np.int16)
    record("indextts cond", lambda: list(eng.run(audio)))
    eng.close()
print("done")
