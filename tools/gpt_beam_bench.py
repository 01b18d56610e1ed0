#!/usr/bin/env python3
"""Cost of a beam-search decode step of the IndexTTS GPT against the batched greedy step over as many rows, in one run.

    python tools/gpt_beam_bench.py [--tokens 256] [--reps 3] [--beams 1,3,5] [--dtype f16] [--small] [--pool [--sampled]]

Full IndexTTS-1.5 size (24 x 1280, 8194 mel codes), synthetic weights, no stop token, so every call decodes --tokens tokens.  For
every beam count B, on one handle: ms per step of generate_batch with nb = B greedy sentences (the yardstick: B rows through the
weights, B private caches, the greedy pick), ms per step of the beam loop with B hypotheses (B rows, one shared cache read
through the ancestor table, the selection), and their ratio.  Median of --reps calls after two warm-up calls (eager, then the
graph capture).  One JSON line per beam count.  --pool adds the pool-mode beam loop (include/mi355tts.h, "beam search with a
finished pool") with B hypotheses, deterministic or with --sampled drawn at temperature 1.0 / top_k 30 / top_p 0.8; with no stop
token it too decodes --tokens tokens, so the three loops differ by their last kernel alone.

    MI355TTS_LIB=<another build> python tools/gpt_beam_bench.py --existing --tag parent [--reps 15]

--existing is the A/B form for two builds of the library in one job (MI355TTS_LIB names the build, mi355tts/_lib.py): ms per step
of the three steps an earlier build has too — generate_batch greedy, generate_batch sampled (temperature 1.0, top_k 30, top_p 0.8)
and the beam loop — over B rows each, with the spread (max - min) / median of the --reps calls, one JSON line per B labelled --tag.
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
from mi355tts.config import IndexGPTConfig  # noqa: E402
from mi355tts.indextts import IndexGPT, Sampling  # noqa: E402


def timed(fn, reps, spread=False):
    fn(); fn()                                     # eager, then the graph capture
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    med = float(np.median(ts))
    return (med, (max(ts) - min(ts)) / med) if spread else med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--beams", default="1,3,5")
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--small", action="store_true", help="the reduced model (a functional check of this tool, not a measurement)")
    ap.add_argument("--pool", action="store_true", help="also time the pool-mode beam loop")
    ap.add_argument("--sampled", action="store_true", help="with --pool: beam sampling (temperature 1.0, top_k 30, top_p 0.8)")
    ap.add_argument("--existing", action="store_true", help="greedy / sampled / beam steps with their spread, for A/B runs of two builds")
    ap.add_argument("--tag", default="this", help="with --existing: the label of the build in the JSON lines")
    a = ap.parse_args()
    if a.sampled and not a.pool:
        ap.error("--sampled belongs to --pool")
    beams = [int(x) for x in a.beams.split(",")]
    cfg = IndexGPTConfig.small() if a.small else IndexGPTConfig()
    cfg.max_batch = max(beams)
    n_tok = min(a.tokens, cfg.max_mel_pos, cfg.max_seq - 48)
    st = W.synth_state(W.gpt_spec(cfg), 9527, fast=not a.small)
    eng = IndexGPT(cfg, st, dtype=a.dtype)
    conds = W.synth_normal(3, "conds", (1, 32 if not a.small else 4, cfg.hidden), std=0.5)
    text = (np.arange(12, dtype=np.int32) * 5 + 3) % (cfg.text_tokens - 2) + 2
    prompt, _ = eng.concat(conds, eng.text_embed(text), eng.mel_embed(cfg.start_mel_token, 0)[0])
    for B in beams if a.existing else []:
        smp = [Sampling(1.0, 30, 0.8, 1 + b) for b in range(B)]
        runs = {"greedy": lambda: eng.generate_batch([prompt] * B, [n_tok] * B, stop_tokens=[]),
                "sampled": lambda: eng.generate_batch([prompt] * B, [n_tok] * B, stop_tokens=[], sampling=smp),
                "beam": lambda: eng.generate_beam([prompt], [n_tok], B, stop_tokens=[])}
        res = {"lib": a.tag, "rows": B, "tokens": n_tok, "reps": a.reps}
        for name, fn in runs.items():
            t, sp = timed(fn, a.reps, spread=True)
            res[name + "_ms_per_step"] = round(t * 1e3 / n_tok, 4)
            res[name + "_spread_pct"] = round(sp * 100, 3)
        print(json.dumps(res), flush=True)
    for B in [] if a.existing else beams:
        t_batch = timed(lambda: eng.generate_batch([prompt] * B, [n_tok] * B, stop_tokens=[]), a.reps)
        t_beam = timed(lambda: eng.generate_beam([prompt], [n_tok], B, stop_tokens=[]), a.reps)
        # a call = its prompt passes (B for the batch, one for the beam) + n_tok - 1 steps; reported per token like the other tools
        res = {"dtype": a.dtype, "beams": B, "tokens": n_tok,
               "batch_greedy_ms_per_step": round(t_batch * 1e3 / n_tok, 4), "beam_ms_per_step": round(t_beam * 1e3 / n_tok, 4)}
        res["ratio"] = round(res["beam_ms_per_step"] / res["batch_greedy_ms_per_step"], 3)
        if a.pool:
            sp = Sampling(1.0, 30, 0.8, 7) if a.sampled else None
            t_pool = timed(lambda: eng.generate_beam([prompt], [n_tok], B, stop_tokens=[], pool=True, sampling=sp), a.reps)
            res["pool"] = "sampled" if a.sampled else "deterministic"
            res["pool_ms_per_step"] = round(t_pool * 1e3 / n_tok, 4)
            res["pool_over_beam_us"] = round((res["pool_ms_per_step"] - res["beam_ms_per_step"]) * 1e3, 1)
        print(json.dumps(res), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
