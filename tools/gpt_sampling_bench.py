#!/usr/bin/env python3
"""Cost of sampling in the IndexTTS GPT decode step: greedy against seeded temperature / top-k / top-p, in one run.

    python tools/gpt_sampling_bench.py [--tokens 256] [--reps 3] [--batches 1,16] [--dtype f16] [--small]

Full IndexTTS-1.5 size (24 x 1280, 8194 mel codes), synthetic weights, no stop token, so every call decodes --tokens tokens:
  * ms per token of generate_from_prompt / generate_batch, greedy and sampled (upstream's temperature 1.0, top_k 30, top_p
    0.8, and the sampler's longest path: top_k 0, top_p 0.8), median of --reps calls after two warm-up calls (eager, then the
    graph capture);
  * microseconds per launch of the token-choosing kernel alone (HIP events around 200 launches, mi_gpt_bench_pick): the greedy
    pick kernel and the sampler with the same parameters.
One JSON line per batch size.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "text-to-speech-tts-onnx_amd"))

import numpy as np  # noqa: E402

from mi355tts import _lib  # noqa: E402
from mi355tts import weights as W  # noqa: E402
from mi355tts.config import IndexGPTConfig  # noqa: E402
from mi355tts.indextts import IndexGPT, Sampling  # noqa: E402

MODES = (("greedy", None), ("sampled_k30_p0.8", Sampling(1.0, 30, 0.8, 1)), ("sampled_k0_p0.8", Sampling(1.0, 0, 0.8, 1)))


def timed(fn, reps):
    fn(); fn()                                     # eager, then the graph capture
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def pick_us(eng, nb, sp, iters=200):
    us = C.c_double(0.0)
    if sp is None:
        args = (None, None, None)
    else:
        T = np.full(nb, sp.temperature, np.float32); K = np.full(nb, sp.top_k, np.int32); P = np.full(nb, sp.top_p, np.float32)
        args = (T.ctypes.data, K.ctypes.data, P.ctypes.data)
    _lib.check(_lib.load().mi_gpt_bench_pick(eng._h, nb, iters, *args, C.byref(us)), "mi_gpt_bench_pick")
    return us.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--small", action="store_true", help="the reduced model (a functional check of this tool, not a measurement)")
    a = ap.parse_args()
    nbs = [int(x) for x in a.batches.split(",")]
    cfg = IndexGPTConfig.small() if a.small else IndexGPTConfig()
    cfg.max_batch = max(nbs)
    n_tok = min(a.tokens, cfg.max_mel_pos, cfg.max_seq - 48)
    st = W.synth_state(W.gpt_spec(cfg), 9527, fast=not a.small)
    eng = IndexGPT(cfg, st, dtype=a.dtype)
    conds = W.synth_normal(3, "conds", (1, 32 if not a.small else 4, cfg.hidden), std=0.5)
    text = (np.arange(12, dtype=np.int32) * 5 + 3) % (cfg.text_tokens - 2) + 2
    prompt, _ = eng.concat(conds, eng.text_embed(text), eng.mel_embed(cfg.start_mel_token, 0)[0])
    for nb in nbs:
        res = {"dtype": a.dtype, "sentences": nb, "tokens": n_tok}
        for name, sp in MODES:
            if nb == 1:
                ones = np.ones((1, cfg.mel_codes), np.float32)
                fn = lambda sp=sp: eng.generate_from_prompt(prompt, n_tok, stop_tokens=[], repeat_penality=ones.copy(), sampling=sp)
            else:
                smp = None if sp is None else [Sampling(sp.temperature, sp.top_k, sp.top_p, sp.seed + b) for b in range(nb)]
                fn = lambda smp=smp: eng.generate_batch([prompt] * nb, [n_tok] * nb, stop_tokens=[], sampling=smp)
            t = timed(fn, a.reps)
            res[name] = {"ms_per_token": round(t * 1e3 / n_tok, 4), "kernel_us": round(pick_us(eng, nb, sp), 2)}
        g = res["greedy"]["ms_per_token"]
        for name, _ in MODES[1:]:
            res[name]["vs_greedy_pct"] = round((res[name]["ms_per_token"] / g - 1.0) * 100.0, 2)
        print(json.dumps(res), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
