#!/usr/bin/env python3
"""Do two builds of the library compute the same IndexTTS GPT outputs, bit for bit?

    MI355TTS_LIB=<library A> python tools/gpt_ab_dump.py --out a.npz        (on the GPU, once per library)
    MI355TTS_LIB=<library B> python tools/gpt_ab_dump.py --out b.npz
    python tools/gpt_ab_dump.py --compare a.npz b.npz                       (on the CPU)

Drives the library named by MI355TTS_LIB (default: the in-tree build; another commit's comes from `build.py --variant NAME` in
a worktree of it) with fixed seeds and synthetic weights and writes every output to one .npz: tokens, last_hidden_state rows,
logits, penalty vectors, beam scores, n_out, queue stats.  --compare requires the two files to hold the same arrays, equal bit
for bit.  MI355TTS_NO_GRAPH=1 is read by the library when a handle is created: run the dump once more with it for the eager path.

The model is the smallest that reaches every attention body and decode linear: hidden 128, 2 heads, 2 layers, inner 256, 96 mel
codes, max_seq 384.  Prompts of 70 and 5 rows with 200 new tokens: the key counts cross 64 (one attention pass per wave) and 256
(the four waves' stride) during the decode.  Entries, each in f32, f16 and bf16: mi_gpt_step with and without mask, generate,
generate_sampled, generate_batch at nb = 3 and 20, generate_queue with 7 sentences in 3 slots, generate_beam at B = 1 and 3
with nb = 2.  Not a pytest test: it needs a second build that a clean checkout does not have.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "text-to-speech-tts-onnx_amd"))

import numpy as np  # noqa: E402

N_NEW = 200


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        x, y = a[k], b[k]
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            bad.append(k)
    print(f"{pa} vs {pb}: {len(a.files)} arrays, " + ("all equal bit for bit" if not bad else "DIFFER: " + " ".join(bad)))
    return 1 if bad else 0


def dump(out):
    from mi355tts import _lib
    from mi355tts import weights as W
    from mi355tts.config import IndexGPTConfig
    from mi355tts.indextts import IndexGPT, Sampling

    def config(max_batch):
        return IndexGPTConfig(hidden=128, layers=2, heads=2, inner=256, mel_codes=96, text_tokens=40, max_mel_pos=N_NEW + 8,
                              max_text_pos=24, max_seq=384, max_batch=max_batch, start_mel_token=94, stop_mel_token=95,
                              max_generate_length=N_NEW)

    cfg = config(20)
    state = W.synth_state(W.gpt_spec(cfg), 9527)
    prompt = lambda i: W.synth_normal(100 + i, "prompt", (1, 5 if i % 2 else 70, cfg.hidden), std=0.5)
    pen0 = lambda nb: 1.0 - 0.25 * (W.synth_normal(7, "pen", (nb, cfg.mel_codes)) > 1.0).astype(np.float32)
    res = {}

    def put(key, seqs, pen=None):                  # seqs: (tokens, hidden[, score]) per sentence
        for i, s in enumerate(seqs):
            res[f"{key}/n_out{i}"] = np.asarray(len(s[0]), np.int32)
            res[f"{key}/tokens{i}"], res[f"{key}/hidden{i}"] = s[0], s[1]
            if len(s) > 2:
                res[f"{key}/score{i}"] = np.asarray(s[2], np.float32)
        if pen is not None:
            res[f"{key}/penalty"] = pen

    for dt in ("f32", "f16", "bf16"):
        eng = IndexGPT(cfg, state, dtype=dt)
        for mask in (1, 0):                        # a 70-row pass, a one-row step on the decode kernels, a one-row masked step
            eng.reset()
            steps = [eng.step(prompt(0), pen0(1), mask, True), eng.step(prompt(1)[:, :1], None, 0, True),
                     eng.step(prompt(3)[:, :1], None, 1, True)]
            for i, (_, last, tok, logits) in enumerate(steps):
                res[f"{dt}/step_mask{mask}/{i}/last"], res[f"{dt}/step_mask{mask}/{i}/token"] = last, tok
                res[f"{dt}/step_mask{mask}/{i}/logits"] = logits
        eng.reset()
        for i in (0, 1):
            t, h, p = eng.generate_from_prompt(prompt(i), N_NEW, stop_tokens=[], repeat_penality=pen0(1))
            put(f"{dt}/generate{i}", [(t, h)], p)
            t, h, p = eng.generate_from_prompt(prompt(i), N_NEW, stop_tokens=[], repeat_penality=pen0(1),
                                               sampling=Sampling(0.9, 20, 0.85, 1234 + i))
            put(f"{dt}/generate_sampled{i}", [(t, h)], p)
        for nb in (3, 20):
            ps, mx = [prompt(i) for i in range(nb)], [N_NEW - 9 * (i % 4) for i in range(nb)]
            put(f"{dt}/batch{nb}", *eng.generate_batch(ps, mx, stop_tokens=[], repeat_penality=pen0(nb)))
            samp = [None if i % 3 == 2 else Sampling(1.1, 12 + i, 0.9, 77 + i) for i in range(nb)]
            put(f"{dt}/batch_sampled{nb}", *eng.generate_batch(ps, mx, stop_tokens=[7], sampling=samp))
        for B in (1, 3):
            put(f"{dt}/beam{B}", *eng.generate_beam([prompt(0), prompt(1)], [N_NEW, N_NEW - 30], B, stop_tokens=[],
                                                    repeat_penality=pen0(2)))
        eng.close()
        q = IndexGPT(config(3), state, dtype=dt)   # the queue takes min(max_batch, n) slots
        ps, mx = [prompt(i) for i in range(7)], [N_NEW, 40, 0, 120, 64, N_NEW, 17]
        for name, samp in (("queue", None), ("queue_sampled", [Sampling(0.8, 25, 0.9, 5 + i) for i in range(7)])):
            seqs, stats = q.generate_queue(ps, mx, stop_tokens=[], sampling=samp, return_stats=True)
            put(f"{dt}/{name}", seqs)
            res[f"{dt}/{name}/stats"] = np.asarray([stats["steps"], stats["passes"]], np.int32)
        q.close()
    np.savez(out, **{k.replace('/', '.'): v for k, v in res.items()})
    print(f"{_lib.lib_path()} (MI355TTS_NO_GRAPH={os.environ.get('MI355TTS_NO_GRAPH', '')}): {len(res)} arrays -> {out}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    if not a.out:
        ap.error("--out FILE or --compare A B")
    dump(a.out)
