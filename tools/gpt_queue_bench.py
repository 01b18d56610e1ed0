#!/usr/bin/env python3
"""The sentence queue of the IndexTTS GPT against lock-step batches of the same sentences, in one run.

    python tools/gpt_queue_bench.py [--sentences 64] [--slots 16] [--rows 100] [--lo 60] [--hi 240] [--dtype f16] [--small]
                                    [--beams B [--pool [--sampled]]]

Full IndexTTS-1.5 size (24 x 1280, 8194 mel codes), synthetic weights, --sentences prompts of --rows rows each, max_new seeded-
uniform in [--lo, --hi], no stop token, so every sentence decodes exactly its limit.  Three measurements on one handle, each the
median wall time of three calls after one warm call (eager steps and graph captures), with the spread (max - min) / median:
  (a) generate_queue over all sentences (slots refilled, prompt passes packed);
  (b) the yardstick: generate_batch over index-order groups of --slots sentences (lock-step, prompt passes one by one);
  (c) prompt passes only, --slots sentences with max_new = 1: through generate_queue (packed) and generate_batch (one by one).
Beside (a) and (b): the decode steps the host model of each schedule predicts (queue_schedule / lockstep_steps) and, for (a),
the steps the entry reports.  One JSON line per measurement and a summary line.

--beams B: beam search.  (a) is generate_queue(beams=B): the queue over the --slots // B groups; (b) is generate_beam over
index-order groups of --slots // B sentences; the host models are queue_schedule(..., beams=B) and lockstep_steps over
--slots // B; (c) compares the packed pass with one selection-0 launch against generate_beam's one-by-one prompt passes.

--beams B --pool [--sampled]: pool mode ("beam search with a finished pool"; --sampled: Sampling(1.0, 30, 0.8, 1001 + i) for
sentence i, upstream IndexTTS' decode configuration).  (a) is generate_queue(beams=B, pool=True), (b) generate_beam(pool=True)
over the same index-order groups, with the same prompts and limits.  Without stop ids a pool search runs max_new selections and
returns max_new codes, so the host models are the ones above.
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
from mi355tts.indextts import IndexGPT, Sampling, lockstep_steps, queue_schedule  # noqa: E402


def timed(fn):
    fn()                                           # warm: eager first steps, graph captures
    ts = []
    for _ in range(3):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    med = float(np.median(ts))
    return med, (max(ts) - min(ts)) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=64)
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--rows", type=int, default=100)
    ap.add_argument("--lo", type=int, default=60)
    ap.add_argument("--hi", type=int, default=240)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--beams", type=int, default=None, help="beam search with B hypotheses per sentence (1..8): groups of B slots")
    ap.add_argument("--pool", action="store_true", help="with --beams: pool mode (generate_queue / generate_beam with pool=True)")
    ap.add_argument("--sampled", action="store_true", help="with --pool: beam sampling, top_k 30, top_p 0.8, seed 1001 + index")
    ap.add_argument("--small", action="store_true", help="the reduced model (a functional check of this tool, not a measurement)")
    a = ap.parse_args()
    cfg = IndexGPTConfig.small() if a.small else IndexGPTConfig()
    n_cond = 4 if a.small else 32
    if a.small:
        cfg.max_seq, cfg.max_mel_pos, cfg.max_text_pos = 512, 300, 130
    cfg.max_batch = a.slots
    n_text = a.rows - n_cond - 3
    assert n_text >= 0 and n_text + 2 <= cfg.max_text_pos and a.rows + a.hi - 1 <= cfg.max_seq and a.hi <= cfg.max_mel_pos
    st = W.synth_state(W.gpt_spec(cfg), 9527, fast=not a.small)
    eng = IndexGPT(cfg, st, dtype=a.dtype)
    mel0 = eng.mel_embed(cfg.start_mel_token, 0)[0]
    prompts = []
    for i in range(a.sentences):
        conds = W.synth_normal(3 + i, "conds", (1, n_cond, cfg.hidden), std=0.5)
        text = (np.arange(n_text, dtype=np.int32) * 5 + 3 + i) % (cfg.text_tokens - 2) + 2
        prompts.append(eng.concat(conds, eng.text_embed(text), mel0)[0])
    limits = np.random.default_rng(a.seed).integers(a.lo, a.hi + 1, a.sentences).tolist()
    rows = [a.rows] * a.sentences
    base = {"dtype": a.dtype, "sentences": a.sentences, "slots": a.slots, "rows": a.rows, "tokens": int(sum(limits))}
    B = a.beams
    if B is not None:
        assert 1 <= B <= 8 and B <= a.slots, "--beams must be in 1..8 and at most --slots"
        base["beams"] = B
    assert not a.pool or B is not None, "--pool is a beam mode: give --beams"
    assert not a.sampled or a.pool, "--sampled belongs to --pool"
    per = a.slots if B is None else a.slots // B       # sentences decoding together
    qkw = {} if B is None else {"beams": B}
    samp = [Sampling(1.0, 30, 0.8, 1001 + i) for i in range(a.sentences)] if a.sampled else None
    if a.pool:
        base["pool"] = "sampled" if a.sampled else "deterministic"
        qkw["pool"] = True

    def skw(lo, hi):                                   # the sampling keyword of sentences lo .. hi - 1
        return {"sampling": samp[lo:hi]} if a.sampled else {}

    stats = {}

    def run_queue():
        _, s = eng.generate_queue(prompts, limits, stop_tokens=[], return_stats=True, **qkw, **skw(0, a.sentences))
        stats.update(s)

    def batch(ps, ls, lo=0):
        if B is None:
            eng.generate_batch(ps, ls, stop_tokens=[])
        elif a.pool:
            eng.generate_beam(ps, ls, B, stop_tokens=[], pool=True, **skw(lo, lo + len(ps)))
        else:
            eng.generate_beam(ps, ls, B, stop_tokens=[])

    def run_groups():
        for g in range(0, a.sentences, per):
            batch(prompts[g:g + per], limits[g:g + per], g)

    t_q, sp_q = timed(run_queue)
    q_steps, q_passes = queue_schedule(rows, limits, limits, a.slots, cfg.max_seq, beams=B or 1)
    ra = dict(base, what="a: generate_queue", seconds=round(t_q, 4), spread=round(sp_q, 4), codes_per_s=round(sum(limits) / t_q, 1),
              model_steps=q_steps, model_passes=len(q_passes), steps=stats["steps"], passes=stats["passes"])
    print(json.dumps(ra), flush=True)
    t_b, sp_b = timed(run_groups)
    b_steps = lockstep_steps(limits, per)
    rb = dict(base, what="b: generate_batch, index-order groups" if B is None else "b: generate_beam, index-order groups" + (" (pool)" if a.pool else ""), seconds=round(t_b, 4), spread=round(sp_b, 4),
              codes_per_s=round(sum(limits) / t_b, 1), model_steps=b_steps, prompt_passes=a.sentences)
    print(json.dumps(rb), flush=True)
    k = min(per, a.sentences)
    t_pp, sp_pp = timed(lambda: eng.generate_queue(prompts[:k], [1] * k, stop_tokens=[], **qkw, **skw(0, k)))
    t_p1, sp_p1 = timed(lambda: batch(prompts[:k], [1] * k))
    rc = dict(base, what="c: prompt passes only", prompts=k, packed_seconds=round(t_pp, 5), packed_spread=round(sp_pp, 4),
              packed_passes=len(queue_schedule(rows[:k], [1] * k, [1] * k, a.slots, cfg.max_seq, beams=B or 1)[1]),
              one_by_one_seconds=round(t_p1, 5), one_by_one_spread=round(sp_p1, 4), ratio=round(t_p1 / t_pp, 3))
    print(json.dumps(rc), flush=True)
    print(json.dumps(dict(base, what="summary", speedup_a_over_b=round(t_b / t_q, 3), model_step_ratio=round(b_steps / q_steps, 3),
                          spread_max=round(max(sp_q, sp_b), 4), a_beats_b=bool(t_b - t_q > max(sp_q * t_q, sp_b * t_b)),
                          packed_not_slower=bool(t_pp <= t_p1 + max(sp_pp * t_pp, sp_p1 * t_p1)))), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
