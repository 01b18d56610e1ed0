#!/usr/bin/env python3
"""Time to first audio and total time of stream_synthesize against the blocking pair, in one process.

    python tools/indextts_stream_bench.py [--dtype f16] [--small] [--cases single,queue] [--chunks 16,32,64] [--halos 0,16]

IndexTTS-1.5 size (GPT 24 x 1280, the graph-F vocoder), synthetic weights, no stop token, so every sentence decodes exactly its
limit; one voice.  Two cases:
  single: 1 sentence of 256 codes in 1 slot;
  queue:  64 sentences of seeded-uniform 60 - 240 codes through 16 slots (the workload of tools/gpt_queue_bench.py).
For each case, on one pair of handles:
  blocking: generate_queue then ONE run_latent_voices over all sentences; the first sample exists when both have returned, so
            its time to first audio IS its total;
  stream:   stream_synthesize at every (chunk, halo) of --chunks x --halos, halo 0 standing for the structural one
            (BigVGANConfig.halo_frames()); first = wall time to the first chunk, total = to the last.
Every figure is the median of three runs after one warm run (eager first steps, graph captures, workspace growth), with the
spread (max - min) / median.  One JSON line per measurement.
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
from mi355tts.config import BigVGANConfig, IndexGPTConfig  # noqa: E402
from mi355tts.indextts import IndexGPT, stream_synthesize  # noqa: E402


def med(ts):
    m = float(np.median(ts))
    return round(m, 5), round((max(ts) - min(ts)) / m, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--small", action="store_true", help="reduced models (a functional check of this tool, not a measurement)")
    ap.add_argument("--cases", default="single,queue")
    ap.add_argument("--chunks", default="16,32,64")
    ap.add_argument("--halos", default="0,16", help="0 = the structural halo")
    ap.add_argument("--rows", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if a.small:
        gcfg = IndexGPTConfig.small()
        gcfg.max_seq, gcfg.max_mel_pos, gcfg.max_text_pos = 512, 300, 130
        vcfg = BigVGANConfig(num_mels=gcfg.hidden, upsample_initial_channel=32, upsample_rates=(4, 2), upsample_kernel_sizes=(8, 4),
                             use_bias_at_final=True, pre_layernorm=True, speaker_cond=True)
        n_cond = 4
    else:
        gcfg, vcfg, n_cond = IndexGPTConfig(), BigVGANConfig.indextts(), 32
    H = vcfg.halo_frames()
    voc = BigVGANVocoder(vcfg, W.synth_state(W.bigvgan_spec(vcfg), 9527, fast=not a.small), dtype=a.dtype)
    sizes = [vcfg.stage_channels(i) for i in range(vcfg.num_upsamples)] + [vcfg.upsample_initial_channel]
    voices = [[W.synth_normal(100 + i, "cond", (n,), std=0.2) for i, n in enumerate(sizes)]]
    gst = W.synth_state(W.gpt_spec(gcfg), 9527, fast=not a.small)
    n_text = a.rows - n_cond - 3
    for case in a.cases.split(","):
        if case == "single":
            n, slots, limits = 1, 1, [256]
        else:
            n, slots = 64, 16
            limits = np.random.default_rng(a.seed).integers(60, 241, n).tolist()
        gcfg.max_batch = slots
        assert n_text >= 0 and a.rows + max(limits) - 1 <= gcfg.max_seq and max(limits) <= gcfg.max_mel_pos
        gpt = IndexGPT(gcfg, gst, dtype=a.dtype)
        mel0 = gpt.mel_embed(gcfg.start_mel_token, 0)[0]
        prompts = []
        for i in range(n):
            conds = W.synth_normal(3 + i, "conds", (1, n_cond, gcfg.hidden), std=0.5)
            text = (np.arange(n_text, dtype=np.int32) * 5 + 3 + i) % (gcfg.text_tokens - 2) + 2
            prompts.append(gpt.concat(conds, gpt.text_embed(text), mel0)[0])
        base = {"case": case, "dtype": a.dtype, "sentences": n, "slots": slots, "codes": int(sum(limits)), "structural_halo": H}

        def blocking():
            t0 = time.perf_counter()
            res = gpt.generate_queue(prompts, limits, stop_tokens=[])
            t1 = time.perf_counter()
            voc.run_latent_voices([h for _, h in res], voices, [0] * n)
            return t1 - t0, time.perf_counter() - t0

        blocking()
        runs = [blocking() for _ in range(3)]
        (dm, ds), (tm, ts) = med([r[0] for r in runs]), med([r[1] for r in runs])
        print(json.dumps(dict(base, what="blocking: generate_queue + run_latent_voices", decode_s=dm, decode_spread=ds, first_s=tm,
                              total_s=tm, total_spread=ts)), flush=True)
        blocking_total = tm
        for halo in [int(x) for x in a.halos.split(",")]:
            for chunk in [int(x) for x in a.chunks.split(",")]:
                def stream():
                    t0 = time.perf_counter()
                    first, k, samples = None, 0, 0
                    for _, _, c, _ in stream_synthesize(gpt, voc, prompts, limits, voices, [0] * n, chunk=chunk, halo=halo or None,
                                                        stop_tokens=[]):
                        if first is None:
                            first = time.perf_counter() - t0
                        k += 1
                        samples += c.size
                    return first, time.perf_counter() - t0, k, samples
                stream()
                runs = [stream() for _ in range(3)]
                assert runs[0][3] == sum((m - 2) * vcfg.hop + 30 for m in limits)
                (fm, fs), (tm, ts) = med([r[0] for r in runs]), med([r[1] for r in runs])
                print(json.dumps(dict(base, what="stream_synthesize", chunk=chunk, halo=halo or H, chunks=runs[0][2], first_s=fm,
                                      first_spread=fs, total_s=tm, total_spread=ts, first_vs_blocking=round(fm / blocking_total, 4),
                                      total_vs_blocking=round(tm / blocking_total, 4))), flush=True)
        gpt.close()
    voc.close()


if __name__ == "__main__":
    main()
