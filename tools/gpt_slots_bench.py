#!/usr/bin/env python3
"""Cost of a batched decode step of the IndexTTS GPT against the number of slots, up to 64, in one run.

    python tools/gpt_slots_bench.py [--nb 1,8,16,17,32,48,64] [--max-batch 64] [--tokens 256] [--rows 100] [--dtype f16] [--weights q8] [--small]

Full IndexTTS-1.5 size (24 x 1280, 8194 mel codes), synthetic weights, ONE handle with --max-batch slots.  For every nb:
generate_batch with nb prompts of --rows rows, --tokens tokens per call, no stop token, so every sentence decodes exactly
--tokens tokens.  The median wall time of three calls after two warm calls (eager first steps, then the graph capture) and the
spread (max - min) / median; the prompt passes are taken out with a max_new = 1 call timed the same way (the call is nb prompt
passes + tokens - 1 decode steps), as tools/gpt_queue_bench.py (c) does:
    ms_per_step = (t_call - t_prompts) / (tokens - 1),  codes_per_s = nb * tokens / t_call.
The family split (linears / attention / rest = the row norms; the token choice carries no profiler scope) comes from one more call with the profiler on
(eager launches timed by events; --prof-tokens tokens, the max_new = 1 call's share subtracted): per-launch event times, so their
sum exceeds the replayed graph's step — read it as shares.  One JSON line per nb.
--max-batch 16 with --nb 1,8,16 runs on a library built from an older commit (MI355TTS_LIB) as well: the yardstick P.
--weights q8: the handle holds its six matrix kinds as per-channel uint8 (IndexGPT(weights="q8"), --dtype f16).  Every line carries
the handle's mi_gpt_weight_bytes where the library has it.
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
from mi355tts.config import IndexGPTConfig  # noqa: E402
from mi355tts.indextts import IndexGPT  # noqa: E402

FAMILIES = ("conv_gemm", "attn", "norm", "other")


def timed(fn):
    fn(); fn()                                     # eager, then the graph capture
    ts = []
    for _ in range(3):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    med = float(np.median(ts))
    return med, (max(ts) - min(ts)) / med


def profiled(fn):
    _lib.prof_reset(); _lib.prof_enable(FAMILIES)
    try:
        fn()
    finally:
        _lib.prof_enable(())
    return {f: _lib.prof_get(f)["ms"] for f in FAMILIES}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", default="1,8,16,17,32,48,64")
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--prof-tokens", type=int, default=33)
    ap.add_argument("--rows", type=int, default=100)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--weights", default=None, choices=["q8"], help="q8: per-channel uint8 weights, dequantised in the kernels")
    ap.add_argument("--small", action="store_true", help="the reduced model (a functional check of this tool, not a measurement)")
    a = ap.parse_args()
    nbs = [int(x) for x in a.nb.split(",")]
    cfg = IndexGPTConfig.small() if a.small else IndexGPTConfig()
    n_cond = 4 if a.small else 32
    if a.small:
        cfg.max_seq, cfg.max_mel_pos, cfg.max_text_pos = 512, 300, 130
    cfg.max_batch = a.max_batch
    n_text = a.rows - n_cond - 3
    n_tok = a.tokens
    assert max(nbs) <= a.max_batch and n_tok >= 2 and 2 <= a.prof_tokens <= n_tok
    assert n_text >= 0 and n_text + 2 <= cfg.max_text_pos and a.rows + n_tok - 1 <= cfg.max_seq and n_tok <= cfg.max_mel_pos
    st = W.synth_state(W.gpt_spec(cfg), 9527, fast=not a.small)
    eng = IndexGPT(cfg, st, dtype=a.dtype, **({"weights": a.weights} if a.weights else {}))
    wbytes = eng.weight_bytes() if hasattr(_lib.load(), "mi_gpt_weight_bytes") else None
    mel0 = eng.mel_embed(cfg.start_mel_token, 0)[0]
    prompts = []
    for i in range(max(nbs)):
        conds = W.synth_normal(3 + i, "conds", (1, n_cond, cfg.hidden), std=0.5)
        text = (np.arange(n_text, dtype=np.int32) * 5 + 3 + i) % (cfg.text_tokens - 2) + 2
        prompts.append(eng.concat(conds, eng.text_embed(text), mel0)[0])
    for nb in nbs:
        run = lambda n: eng.generate_batch(prompts[:nb], [n] * nb, stop_tokens=[])
        t, sp = timed(lambda: run(n_tok))
        t1, sp1 = timed(lambda: run(1))
        step = (t - t1) / (n_tok - 1)
        full, one = profiled(lambda: run(a.prof_tokens)), profiled(lambda: run(1))
        fam = {f: (full[f] - one[f]) / (a.prof_tokens - 1) for f in FAMILIES}
        print(json.dumps({"dtype": a.dtype, "weights": a.weights or a.dtype, "weight_bytes": wbytes, "max_batch": a.max_batch, "nb": nb, "rows": a.rows, "tokens": n_tok,
                          "seconds": round(t, 4), "spread": round(sp, 4), "prompt_seconds": round(t1, 4),
                          "prompt_spread": round(sp1, 4), "ms_per_step": round(step * 1e3, 4),
                          "codes_per_s": round(nb * n_tok / t, 1),
                          "eager_ms_per_step": {"linears": round(fam["conv_gemm"], 4), "attention": round(fam["attn"], 4),
                                                "rest": round(fam["norm"] + fam["other"], 4)}}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
