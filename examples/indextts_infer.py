#!/usr/bin/env python
"""Prompt wav + text in, WAVEX file out: IndexTTS on the MI355X engine's own API.

Three engine objects do what the reference's driver (IndexTTS/Inference_IndexTTS_ONNX.py) spreads over six ONNX Runtime
sessions: `IndexCond.run` (its graph A: prompt audio -> speaker conditioning for the vocoder + the GPT prompt's conditioning
rows), `IndexGPT.generate` (graphs B, C, D and the whole greedy loop over graph E — prompt pass, KV cache, repeat penalty,
stop test — as ONE call whose loop runs on the device), `BigVGANVocoder.run_latent` (graph F: the stacked last hidden
states -> int16 waveform).  `--device-type cuda` keeps the per-sentence tensors on the device between the three calls
(`generate_torch` / `run_latent_torch`); `cpu` passes numpy arrays.  Both forms write the same file.

With no checkpoint on disk the weights are the seeded synthetic ones (`--small`: reduced models for smoke runs): the output
is noise-like audio, but every shape, dtype and call is the real one.  For the reference driver's own call sequence through
`import mi355tts.ort_compat as onnxruntime`, see INTEGRATION.md section 4 and tests/test_gpu_compat.py.

    python examples/indextts_infer.py --prompt prompt.wav --text "..." --out generated.wav [--small] [--device-type cuda]

Decoding is greedy like the reference's unless one of --temperature / --top-k / --top-p / --sample-seed is given: then every mel
code is drawn on the device (`Sampling`, upstream IndexTTS's temperature 1.0 / top_k 30 / top_p 0.8 where not given).
`--takes N` decodes every sentence in N batch slots at once, seeds sample-seed .. sample-seed + N - 1, and writes
<out>_<i>.wav: N takes for the weight traffic of one.
`--num-beams N` decodes every sentence by beam search instead (upstream IndexTTS runs 3 beams): N hypotheses in N batch slots
over one shared KV cache, the most probable one goes to the vocoder.  Beam search is deterministic and does not combine with the
sampling flags.
`--num-beams N --beam-pool [--length-penalty x] [--early-stopping]` is upstream's own beam search: finished hypotheses are kept
in a pool, the search goes on while a running one can still beat them, and the best of the pool goes to the vocoder.  With
`--beam-pool` the sampling flags ARE accepted together with `--num-beams` (beam sampling: `--num-beams 3 --beam-pool --top-k 30
--top-p 0.8` is what upstream runs).  Every sentence starts from a fresh penalty vector; not with --takes or --device-type
cuda.
`--queue` decodes the whole text at once instead of sentence by sentence: every sentence is embedded, `generate_queue` runs them
through `--slots` batch slots (default 8, 1..64) — a slot is refilled as soon as its sentence stops and the prompts admitted
together share one pass over the weights — and `run_latent_ragged` vocodes them in one forward, in order, with the same gap.
Every queued sentence starts from a FRESH penalty vector: the sentences run concurrently, so the carry of the vector from one
sentence to the next that the sentence-by-sentence forms keep (like the reference) does not exist there.  Sampling flags apply
(one seed per sentence: sample-seed + its index); takes do not go through the queue.  `--queue --num-beams N` is beam search
through the queue: every sentence runs as a group of N slots, the queue schedules the `--slots` // N groups, and with `--stream`
a sentence's audio leaves whole, as soon as its group is retired, while the other groups decode.  `--queue --num-beams N
--beam-pool [--top-k 30 --top-p 0.8 --sample-seed s] [--length-penalty x] [--early-stopping] [--stream]` is upstream's decode
configuration through the queue: the groups run the pool-mode search (one seed per sentence: sample-seed + its index), and a
sentence's result is what `--beam-pool` gives for it alone.
With `--queue`, `--prompt a.wav,b.wav,...` is a dialogue: graph A runs once per file, sentence i is spoken by voice i mod V (or by
`--voice-of 0,1,1,0,...`, one index per sentence), every sentence's prompt carries its own voice's conditioning rows, and ONE
`run_latent_voices` call vocodes all of them in order, whatever the mix of voices.  One prompt file is the one-voice case of the
same calls: the same output file as before.
`--queue --stream` returns audio while the queue is still decoding: `stream_synthesize` drives the queue as a session and, after
every round of decode steps, vocodes `--chunk` frames (default 32) of every sentence that has them ready, with `--halo` frames of
context at each cut (default: the vocoder's receptive field, `BigVGANConfig.halo_frames()`, with which the samples are those of the
whole sentence's forward; fewer trade accuracy for work), in ONE `run_latent_windows_torch` call for all sentences and voices.  The
chunks are assembled here and the file has the layout of `--queue`; the wall time to the first chunk and to the last is printed.
"""
import argparse
import dataclasses
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "text-to-speech-tts-onnx_amd"))

from mi355tts import audio_io, weights                                       # noqa: E402
from mi355tts.bigvgan import BigVGANVocoder                                   # noqa: E402
from mi355tts.config import BigVGANConfig, IndexCondConfig, IndexGPTConfig    # noqa: E402
from mi355tts.indextts import IndexCond, IndexGPT, Sampling, stream_synthesize    # noqa: E402
from mi355tts.indextts_text import TextNormalizer, TextTokenizer              # noqa: E402


def build_tokenizer(model_file):
    import sentencepiece as spm
    sp = spm.SentencePieceProcessor(model_file=model_file)
    norm = TextNormalizer()
    try:
        norm.load()                            # WeTextProcessing / wetext when installed (number / date verbalisation is theirs alone)
    except ImportError:
        class Passthrough:
            def normalize(self, t):
                return t
        norm = TextNormalizer(zh=Passthrough(), en=Passthrough())
        print("WeTextProcessing is not installed: text goes to the tokenizer un-verbalised")
    return sp, TextTokenizer(sp, norm)


def build_engines(args, vocab):
    if args.small:
        gcfg = dataclasses.replace(IndexGPTConfig.small(), text_tokens=vocab + 2, max_text_pos=130, max_seq=512, max_mel_pos=300,
                                   max_generate_length=args.max_generate_length or 200)
        ccfg = IndexCondConfig.small()
        vcfg = BigVGANConfig(num_mels=gcfg.hidden, upsample_initial_channel=ccfg.voc_initial, upsample_rates=(4, 2),
                             upsample_kernel_sizes=(8, 4), use_bias_at_final=True, pre_layernorm=True, speaker_cond=True)
    else:
        gcfg, ccfg, vcfg = IndexGPTConfig(), IndexCondConfig(), BigVGANConfig.indextts()
        if args.max_generate_length:
            gcfg = dataclasses.replace(gcfg, max_generate_length=args.max_generate_length)
    # batch slots: one sentence at a time here, so its takes or its beams (sentences per batch x beams in general)
    gcfg = dataclasses.replace(gcfg, max_batch=max(gcfg.max_batch, args.takes, args.num_beams, args.slots if args.queue else 1))
    fast = not args.small
    state = lambda spec: weights.synth_state(spec, args.seed, fast=fast)
    cond = IndexCond(ccfg, state(weights.cond_spec(ccfg)))
    gpt = IndexGPT(gcfg, state(weights.gpt_spec(gcfg)), dtype=args.dtype, weights=args.gpt_weights)
    voc = BigVGANVocoder(vcfg, state(weights.bigvgan_spec(vcfg)), dtype=args.dtype)
    return (gcfg, ccfg, vcfg), (cond, gpt, voc)


MAX_SLOTS = 64                                 # the engine's batch slots (IndexGPTConfig.max_batch)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompt", help="reference audio (RIFF/WAVE); default: a synthetic 3 s tone.  With --queue: a comma-separated list, one file per voice")
    ap.add_argument("--voice-of", default=None, help="with --queue and several prompts: the voice index of every sentence, comma-separated "
                    "(default: sentence i speaks with voice i mod V)")
    ap.add_argument("--text", default="The quick brown fox jumps over the lazy dog. Pack my box with five dozen liquor jugs!")
    ap.add_argument("--out", default="generated.wav")
    ap.add_argument("--tokenizer", default=os.path.join(ROOT, "tests", "golden", "indextts_sp.model"),
                    help="sentencepiece model; default: the small fixture model of this repo")
    ap.add_argument("--dtype", default="f16", choices=["f32", "f16", "bf16"])
    ap.add_argument("--gpt-weights", default=None, choices=["q8"], help="q8: the GPT's linear weights as per-channel uint8, dequantised in the "
                    "kernels (needs --dtype f16; about half the f16 handle's weight bytes)")
    ap.add_argument("--device-type", default="cpu", choices=["cpu", "cuda"], help="cuda: per-sentence tensors stay in HBM between the engine calls")
    ap.add_argument("--small", action="store_true", help="reduced synthetic models (smoke runs)")
    ap.add_argument("--max-generate-length", type=int, default=None)
    ap.add_argument("--ignore-stop", action="store_true", help="decode to the length limit (synthetic weights emit the stop code at random)")
    ap.add_argument("--seed", type=int, default=9527, help="seed of the synthetic weights")
    ap.add_argument("--temperature", type=float, default=None, help="sample the mel codes (default: greedy, like the reference)")
    ap.add_argument("--top-k", type=int, default=None, help="0 = every code")
    ap.add_argument("--top-p", type=float, default=None)
    ap.add_argument("--sample-seed", type=int, default=None, help="seed of the draws (--seed is the synthetic weights')")
    ap.add_argument("--takes", type=int, default=1, help="decode every sentence N times in one batch, seeds sample-seed .. + N - 1; writes <out>_<i>.wav")
    ap.add_argument("--num-beams", type=int, default=1, help="beam search with N hypotheses per sentence (1..8; 1 = greedy)")
    ap.add_argument("--beam-pool", action="store_true", help="with --num-beams: beam search with a pool of finished hypotheses; the sampling flags then combine with it")
    ap.add_argument("--length-penalty", type=float, default=0.0, help="with --beam-pool: a finished hypothesis scores log-probability / length ** x")
    ap.add_argument("--early-stopping", action="store_true", help="with --beam-pool: end as soon as the pool holds --num-beams finished hypotheses")
    ap.add_argument("--queue", action="store_true", help="decode all sentences through the batch slots (refilled as sentences end); "
                    "every sentence starts from a fresh penalty vector")
    ap.add_argument("--slots", type=int, default=8, help=f"batch slots of --queue (1..{MAX_SLOTS})")
    ap.add_argument("--stream", action="store_true", help="with --queue: vocode windows of every sentence while the queue decodes (time to first audio)")
    ap.add_argument("--chunk", type=int, default=32, help="frames per streamed window")
    ap.add_argument("--halo", type=int, default=None, help="context frames at each cut of a streamed window (default: the vocoder's receptive field)")
    args = ap.parse_args(argv)
    if args.stream and not args.queue:
        ap.error("--stream needs --queue (it streams the sentence queue)")
    if args.chunk < 1 or (args.halo is not None and args.halo < 0):
        ap.error("--chunk must be >= 1 and --halo >= 0")
    args.prompts = args.prompt.split(",") if args.prompt else [None]
    if (len(args.prompts) > 1 or args.voice_of is not None) and not args.queue:
        ap.error("several --prompt files / --voice-of need --queue (one run_latent_voices call vocodes the whole dialogue)")
    if args.voice_of is not None:
        try:
            args.voice_of = [int(x) for x in args.voice_of.split(",")]
        except ValueError:
            ap.error("--voice-of takes comma-separated integers")
        if any(not 0 <= x < len(args.prompts) for x in args.voice_of):
            ap.error(f"--voice-of indices must be in 0..{len(args.prompts) - 1} (one --prompt file per voice)")
    if not 1 <= args.slots <= MAX_SLOTS:
        ap.error(f"--slots must be in 1..{MAX_SLOTS} (the engine's batch slots)")
    if args.queue and (args.takes > 1 or args.device_type == "cuda"):
        ap.error("--queue uses the host-array queue call (generate_queue): no --takes, --device-type cpu")
    if not 1 <= args.num_beams <= 8:
        ap.error("--num-beams must be in 1..8")
    if args.queue and args.num_beams > args.slots:
        ap.error("--queue --num-beams N runs every sentence in a group of N slots: --slots must be at least N")
    if not 1 <= args.takes <= MAX_SLOTS:
        ap.error(f"--takes must be in 1..{MAX_SLOTS} (the engine's batch slots)")
    args.sampled = args.takes > 1 or any(v is not None for v in (args.temperature, args.top_k, args.top_p, args.sample_seed))
    if args.beam_pool and (args.takes > 1 or args.device_type == "cuda"):
        ap.error("--beam-pool decodes through the host-array beam calls (sentence by sentence, or --queue): no --takes, --device-type cpu")
    if not args.beam_pool and (args.length_penalty != 0.0 or args.early_stopping):
        ap.error("--length-penalty and --early-stopping belong to --beam-pool")
    if not math.isfinite(args.length_penalty):
        ap.error("--length-penalty must be finite")
    if args.num_beams > 1 and args.sampled and not args.beam_pool:
        ap.error("--num-beams does not combine with --temperature / --top-k / --top-p / --sample-seed / --takes: beam search is deterministic")
    if args.takes > 1 and args.device_type == "cuda":
        ap.error("--takes uses the host-array batch call (generate_batch); run it with --device-type cpu")
    return args


def main():
    args = parse_args()
    sampled = args.sampled
    take_sampling = [Sampling(1.0 if args.temperature is None else args.temperature, 30 if args.top_k is None else args.top_k,
                              0.8 if args.top_p is None else args.top_p, (args.sample_seed or 0) + i)
                     for i in range(args.takes)] if sampled else None

    sp, tokenizer = build_tokenizer(args.tokenizer)
    (gcfg, ccfg, vcfg), (cond, gpt, voc) = build_engines(args, sp.get_piece_size())
    rate = vcfg.sampling_rate
    prompt_audios = [np.asarray(audio_io.load_prompt(f, rate), dtype=np.int16).reshape(-1) if f else
                     (0.1 * 32767 * np.sin(2 * np.pi * 220 * np.arange(3 * rate) / rate)).astype(np.int16) for f in args.prompts]
    on_device = args.device_type == "cuda"
    if on_device:
        import torch
        dev = torch.device("cuda", 0)

    t_start = time.time()
    speakers = []                                                       # per voice: (graph F's conditioning list, the GPT prompt's rows)
    for audio in prompt_audios:                                         # graph A, once per speaker
        voc_cond_flat, latent_rows = cond.run(audio)
        stage, embed = cond.split_conds(voc_cond_flat)
        speakers.append((list(stage) + [embed], latent_rows))
    (*stage_conds, embed_cond), conds_latent = speakers[0]              # the sentence-by-sentence forms speak with the first voice
    stops = [] if args.ignore_stop else [gcfg.stop_mel_token]
    gap = np.zeros((1, 1, int(rate * 0.2)), dtype=np.int16)              # 0.2 s of silence behind every sentence
    if on_device:
        voc_cond_dev = torch.from_numpy(np.concatenate([np.ravel(c) for c in stage_conds] + [np.ravel(embed_cond)]).astype(np.float32)).to(dev)
        penalty_dev = torch.ones(gcfg.mel_codes, dtype=torch.float32, device=dev)     # carried from sentence to sentence, like the host form
    pieces, n_codes = [], 0
    take_pieces = [[] for _ in range(args.takes)]
    take_penalty = None
    sentences = tokenizer.split_sentences(tokenizer.tokenize(args.text))
    if args.queue:
        prompts, budgets = [], []
        voice_of = args.voice_of if args.voice_of is not None else [i % len(speakers) for i in range(len(sentences))]
        if len(voice_of) != len(sentences):
            raise SystemExit(f"--voice-of names {len(voice_of)} sentences, the text has {len(sentences)}")
        for sentence, voice in zip(sentences, voice_of):
            print(f"Queue voice {voice} for '" + "".join(sentence).replace("▁", " ") + "'")
            ids = np.asarray(tokenizer.convert_tokens_to_ids(sentence), dtype=np.int32)
            prompt_rows, prompt_len = gpt.concat(speakers[voice][1][None], gpt.text_embed(ids), gpt.mel_embed(gcfg.start_mel_token, 0)[0])
            prompts.append(prompt_rows)
            budgets.append(max(gcfg.max_generate_length - int(prompt_len[0]), 0))
        t_dec = time.time()
        q_sampling = [dataclasses.replace(take_sampling[0], seed=take_sampling[0].seed + i) for i in range(len(prompts))] if sampled else None
        # a sentence in a group of N slots, the queue over slots // N groups; --beam-pool: the groups run the pool-mode search
        q_beams = args.num_beams if args.num_beams > 1 or args.beam_pool else None
        q_pool = dict(pool=True, length_penalty=args.length_penalty, early_stopping=args.early_stopping) if args.beam_pool else {}
        if args.stream:
            chunks, t_first = {}, None
            for i, first_sample, chunk, last in stream_synthesize(gpt, voc, prompts, budgets, [c for c, _ in speakers], voice_of,
                                                                  chunk=args.chunk, halo=args.halo, stop_tokens=stops, sampling=q_sampling,
                                                                  beams=q_beams, **q_pool):
                if t_first is None:
                    t_first = time.time() - t_dec
                assert first_sample == sum(c.size for c in chunks.get(i, []))
                chunks.setdefault(i, []).append(chunk)
            t_last = time.time() - t_dec
            n_codes = sum((sum(c.size for c in chunks[i]) - 30) // vcfg.hop + 2 for i in chunks)
            n_chunks = sum(len(c) for c in chunks.values())
            print(f"Streamed {n_chunks} chunks of {len(chunks)} sentence(s) in {gcfg.max_batch} slots (chunk {args.chunk}, halo "
                  f"{vcfg.halo_frames() if args.halo is None else args.halo}): first chunk after {1e3 * (t_first or 0.0):.1f} ms, last after {1e3 * t_last:.1f} ms")
            for i in sorted(chunks):
                pieces.append(np.concatenate([np.concatenate(chunks[i]).reshape(1, 1, -1), gap], axis=-1))
            results = []
        else:
            results, q_stats = gpt.generate_queue(prompts, budgets, stop_tokens=stops, sampling=q_sampling, beams=q_beams,
                                                  return_stats=True, **q_pool)
            results = [r[:2] for r in results]                       # (tokens, hidden[, score])
            n_codes = sum(h.shape[0] for _, h in results)
            print(f"Decode Speed: {n_codes / max(time.time() - t_dec, 1e-9):.3f} tokens/s ({n_codes} tokens, {len(prompts)} sentences in "
                  f"{gcfg.max_batch} slots: {q_stats['steps']} decode steps, {q_stats['passes']} prompt passes)")
        keep = [i for i, (_, h) in enumerate(results) if h.shape[0] >= 3]         # the vocoder needs three codes
        if keep:                                                     # one forward for every voice in flight
            for wav in voc.run_latent_voices([results[i][1] for i in keep], [c for c, _ in speakers], [voice_of[i] for i in keep]):
                pieces.append(np.concatenate([wav, gap], axis=-1))
    for sentence in ([] if args.queue else sentences):
        print("Generate the Voice for '" + "".join(sentence).replace("▁", " ") + "'")
        ids = np.asarray(tokenizer.convert_tokens_to_ids(sentence), dtype=np.int32)
        t_dec = time.time()
        if args.takes > 1:                         # the same sentence in every slot: one pass over the weights per step for all takes
            prompt_rows, prompt_len = gpt.concat(conds_latent[None], gpt.text_embed(ids), gpt.mel_embed(gcfg.start_mel_token, 0)[0])
            budget = gcfg.max_generate_length - int(prompt_len[0])
            results, take_penalty = gpt.generate_batch([prompt_rows] * args.takes, [budget] * args.takes, stop_tokens=stops,
                                                       repeat_penality=take_penalty, sampling=take_sampling)
            n = sum(h.shape[0] for _, h in results)
            print(f"Decode Speed: {n / max(time.time() - t_dec, 1e-9):.3f} tokens/s ({n} tokens in {args.takes} takes)")
            n_codes += n
            for i, (_, hidden) in enumerate(results):
                if hidden.shape[0] >= 3:
                    take_pieces[i].append(np.concatenate([voc.run_latent(hidden, list(stage_conds) + [embed_cond]), gap], axis=-1))
            continue
        if args.beam_pool:
            prompt_rows, prompt_len = gpt.concat(conds_latent[None], gpt.text_embed(ids), gpt.mel_embed(gcfg.start_mel_token, 0)[0])
            budget = gcfg.max_generate_length - int(prompt_len[0])
            res, _ = gpt.generate_beam([prompt_rows], [budget], args.num_beams, stop_tokens=stops, pool=True,
                                       length_penalty=args.length_penalty, early_stopping=args.early_stopping,
                                       sampling=take_sampling[0] if sampled else None)
            hidden = res[0][1]
            n = hidden.shape[0]
        elif on_device:
            prompt_rows, prompt_len = gpt.concat(conds_latent[None], gpt.text_embed(ids), gpt.mel_embed(gcfg.start_mel_token, 0)[0])
            budget = gcfg.max_generate_length - int(prompt_len[0])
            codes = torch.zeros(max(budget, 1), dtype=torch.int32, device=dev)
            hidden = torch.zeros((max(budget, 1), gcfg.hidden), dtype=torch.float32, device=dev)
            n = gpt.generate_torch(torch.from_numpy(prompt_rows[0]).to(dev), budget, codes, hidden, stop_tokens=stops, repeat_penality=penalty_dev,
                                   sampling=take_sampling[0] if sampled else None, beams=args.num_beams)
            hidden = hidden[:n].contiguous()
        else:
            _, hidden, _ = gpt.generate(conds_latent[None], ids, stop_tokens=stops, sampling=take_sampling[0] if sampled else None,
                                        beams=args.num_beams)
            n = hidden.shape[0]
        print(f"Decode Speed: {n / max(time.time() - t_dec, 1e-9):.3f} tokens/s ({n} tokens)")
        n_codes += n
        if n >= 3:                                 # the vocoder needs three codes: (n - 2) * hop + 30 samples
            if on_device:
                wav = voc.run_latent_torch(hidden, voc_cond_dev).cpu().numpy()
            else:
                wav = voc.run_latent(hidden, list(stage_conds) + [embed_cond])
            pieces.append(np.concatenate([wav, gap], axis=-1))
    elapsed = time.time() - t_start
    if args.takes > 1:
        base, ext = os.path.splitext(args.out)
        secs = 0.0
        for i, tp in enumerate(take_pieces):
            out = np.concatenate(tp, axis=-1) if tp else gap
            audio_io.write_wavex(f"{base}_{i}{ext}", out.reshape(-1), rate)
            secs += out.size / rate
        print(f"{base}_0{ext} .. {base}_{args.takes - 1}{ext}: {len(sentences)} sentence(s) x {args.takes} takes, {n_codes} mel codes, "
              f"{secs:.2f} s of audio in {elapsed:.3f} s (RTF {elapsed / max(secs, 1e-9):.4f})")
    else:
        out = np.concatenate(pieces, axis=-1) if pieces else gap
        audio_io.write_wavex(args.out, out.reshape(-1), rate)
        secs = out.size / rate
        print(f"{args.out}: {len(sentences)} sentence(s), {n_codes} mel codes, {secs:.2f} s of audio in {elapsed:.3f} s (RTF {elapsed / max(secs, 1e-9):.4f})")
    for e in (cond, gpt, voc):
        e.close()


if __name__ == "__main__":
    main()
