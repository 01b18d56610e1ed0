#!/usr/bin/env python3
"""Cost of a beam-search decode step of the IndexTTS GPT against the batched greedy step over as many rows, in one run.

    python tools/gpt_beam_bench.py [--tokens 256] [--reps 3] [--beams 1,3,5] [--dtype f16] [--small]

Full IndexTTS-1.5 size (24 x 1280, 8194 mel codes), synthetic weights, no stop token, so every call decodes --tokens tokens.  For
every beam count B, on one handle: ms per step of generate_batch with nb = B greedy sentences (the yardstick: B rows through the
weights, B private caches, the greedy pick), ms per step of the beam loop with B hypotheses (B rows, one shared cache read
through the ancestor table, the selection), and their ratio.  Median of --reps calls after two warm-up calls (eager, then the
graph capture).  One JSON line per beam count.
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
from mi355tts.indextts import IndexGPT  # noqa: E402


def timed(fn, reps):
    fn(); fn()                                     # eager, then the graph capture
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--beams", default="1,3,5")
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--small", action="store_true", help="the reduced model (a functional check of this tool, not a measurement)")
    a = ap.parse_args()
    beams = [int(x) for x in a.beams.split(",")]
    cfg = IndexGPTConfig.small() if a.small else IndexGPTConfig()
    cfg.max_batch = max(beams)
    n_tok = min(a.tokens, cfg.max_mel_pos, cfg.max_seq - 48)
    st = W.synth_state(W.gpt_spec(cfg), 9527, fast=not a.small)
    eng = IndexGPT(cfg, st, dtype=a.dtype)
    conds = W.synth_normal(3, "conds", (1, 32 if not a.small else 4, cfg.hidden), std=0.5)
    text = (np.arange(12, dtype=np.int32) * 5 + 3) % (cfg.text_tokens - 2) + 2
    prompt, _ = eng.concat(conds, eng.text_embed(text), eng.mel_embed(cfg.start_mel_token, 0)[0])
    for B in beams:
        t_batch = timed(lambda: eng.generate_batch([prompt] * B, [n_tok] * B, stop_tokens=[]), a.reps)
        t_beam = timed(lambda: eng.generate_beam([prompt], [n_tok], B, stop_tokens=[]), a.reps)
        # a call = its prompt passes (B for the batch, one for the beam) + n_tok - 1 steps; reported per token like the other tools
        res = {"dtype": a.dtype, "beams": B, "tokens": n_tok,
               "batch_greedy_ms_per_step": round(t_batch * 1e3 / n_tok, 4), "beam_ms_per_step": round(t_beam * 1e3 / n_tok, 4)}
        res["ratio"] = round(res["beam_ms_per_step"] / res["batch_greedy_ms_per_step"], 3)
        print(json.dumps(res), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
