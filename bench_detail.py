#!/usr/bin/env python
"""bench_detail.py — everything the bench measures BESIDE the headline line of bench.py: the secondary workloads of the
default run (configs[1] BigVGAN fp16 B = 8, the configs[3] shard, native-fp32 / four-utterance / two-request / façade forms of
configs[2], F5 + BigVGAN), the rocprofv3 --pmc passes that fill `roofline.traffic`, and the stand-alone BigVGAN / IndexTTS
workloads (`bench.py --workload bigvgan|indextts|indextts_f` dispatches here).  Nothing in this file decides `value`."""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np

from bench_common import (ROOT, USER_OPTIONS, HBM_PEAK_GBS, MFMA_F16_PEAK_TF, MFMA_F32_PEAK_TF, dominant_kernel_roofline,
                          bcast_device_blob, max_over_ranks, f5_workload_name, emit, synth_state_threaded, dump_outputs)


def bigvgan_algorithmic_bytes(cfg, B: int, F: int, esz: int) -> float:
    """Layer-granular HBM bytes of one forward: per stage 85*E_i + E_{i-1} + E_i,
    conv_pre, post activation, conv_post, weights once."""
    total = 0.0
    T = F
    e_prev = B * cfg.upsample_initial_channel * T * esz
    total += B * cfg.num_mels * F * 4 + e_prev                      # conv_pre: read mel (fp32), write E_pre
    for i, u in enumerate(cfg.upsample_rates):
        T *= u
        e = B * cfg.stage_channels(i) * T * esz
        total += e_prev + e + 85.0 * e
        e_prev = e
    total += 2 * e_prev                                             # post AA activation
    total += e_prev + B * (T + 30) * 2                              # conv_post -> int16
    from mi355tts.weights import bigvgan_spec
    total += sum(int(np.prod(s)) for _, s, _ in bigvgan_spec(cfg)) * esz
    return total


def cpu_baseline_bigvgan(cfg, state, frames: int):
    """numpy oracle (kind 'port') on a bounded sample of the same workload."""
    from oracle import bigvgan_np as O
    from mi355tts.weights import synth_normal
    mel = synth_normal(11, "mel", (1, cfg.num_mels, frames), std=2.0, mean=-2.0).clip(-11.5, 2.5)
    t0 = time.perf_counter()
    w = O.bigvgan_int16(cfg, state, mel)
    dt = time.perf_counter() - t0
    secs = w.shape[-1] / cfg.sampling_rate
    try:
        from threadpoolctl import threadpool_info
        cores = max([p.get("num_threads", 1) for p in threadpool_info()] + [1])
    except Exception:
        cores = os.cpu_count() or 1
    return {"value": secs / dt, "unit": "audio-s/s", "cores": int(cores), "kind": "port",
            "sample": f"numpy oracle, BigVGAN-v2 fp32, mel (1,{cfg.num_mels},{frames}) = {secs:.2f} s audio in {dt:.1f} s"}



def pmc_traffic(kernel_label: str, dtype: str, U: int, child=None, family=None):
    """`roofline.traffic` of the dominant kernel: fabric-side bytes per launch from rocprofv3 PMC counters, collected as
    MI355X_MICROARCH.md (HBM section) prescribes — FETCH_SIZE and WRITE_SIZE in SEPARATE --pmc passes (they do not fit one
    pass), FETCH_SIZE doubled (gfx950 tallies 128-byte requests at 64 B), WRITE_SIZE as reported (uncalibrated), both in KB.
    The passes run a SHORT child command (tools/pmc_f5_eval.py: one DiT evaluation of the same utterance shape on the same
    engine, ~260 dispatches — a PMC pass costs ~40 ms per dispatch) and the counters of the launches of that kernel are
    averaged.  `family`: a regular expression over the demangled kernel names — every matching instantiation is pooled
    (launch-weighted, as the event timing of a merged roofline row is) and listed on its own in the detail.
    Returns (bytes_per_launch, detail) or (None, reason)."""
    import csv
    import glob
    import re
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if exe is None:
        return None, "rocprofv3 not found"
    if any(k.startswith(("ROCPROF", "ROCP_")) for k in os.environ) or "rocprofiler" in os.environ.get("LD_PRELOAD", ""):
        return None, "bench.py is itself running under a profiler: nested PMC passes skipped"
    base = kernel_label.split("<")[0].strip()
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["TMPDIR"] = "/tmp"
    sums, counts, names, totals, insts = {}, {}, {}, {}, {}
    with tempfile.TemporaryDirectory(prefix="mi355tts_pmc_", dir="/tmp") as td:
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            out = os.path.join(td, ctr)
            cmd = [exe, "--kernel-trace", "--pmc", ctr, "--output-format", "csv", "-d", out, "--", sys.executable,
                   *(child or [os.path.join(ROOT, "tools", "pmc_f5_eval.py"), dtype, str(U), "1"])]
            try:
                r = subprocess.run(cmd, env=env, cwd="/tmp", capture_output=True, text=True, timeout=600)
            except subprocess.TimeoutExpired:
                return None, f"rocprofv3 --pmc {ctr} timed out"
            if r.returncode != 0:
                return None, f"rocprofv3 --pmc {ctr} failed: {r.stderr[-300:]}"
            per = {}
            for f in glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True):
                for row in csv.DictReader(open(f)):
                    if row.get("Counter_Name") != ctr:
                        continue
                    totals[ctr] = totals.get(ctr, 0.0) + float(row["Counter_Value"])
                    nm = re.sub(r"\(.*\)$", "", re.sub(r"^void ", "", row["Kernel_Name"])).replace("mi::", "")
                    if (not re.search(family, nm)) if family else (base not in nm):   # (f16 instantiations stay mangled in the CSV — the demangler does not know _Float16 — but carry the name)
                        continue
                    e = per.setdefault(nm, [0.0, 0])
                    e[0] += float(row["Counter_Value"]); e[1] += 1
            if not per:
                return None, f"no {base} dispatch in the {ctr} pass"
            if family:
                sums[ctr], counts[ctr], names[ctr] = sum(v[0] for v in per.values()), sum(v[1] for v in per.values()), family
                insts[ctr] = {k: v[0] * 1024.0 * (2.0 if ctr == "FETCH_SIZE" else 1.0) / v[1] for k, v in per.items()}
                continue
            nm = max(per, key=lambda k: per[k][1])              # the instantiation with the most launches
            sums[ctr], counts[ctr], names[ctr] = per[nm][0], per[nm][1], nm
    fetch = 2.0 * sums["FETCH_SIZE"] * 1024.0 / counts["FETCH_SIZE"]
    write = sums["WRITE_SIZE"] * 1024.0 / counts["WRITE_SIZE"]
    return fetch + write, {"kernel": names["FETCH_SIZE"], "launches_sampled": counts["FETCH_SIZE"],
                           "fetch_bytes_per_launch_x2_corrected": fetch, "write_bytes_per_launch": write,
                           "whole_command_bytes": 2.0 * totals.get("FETCH_SIZE", 0.0) * 1024.0 + totals.get("WRITE_SIZE", 0.0) * 1024.0,
                           **({"per_instantiation_bytes_per_launch": {k: insts["FETCH_SIZE"][k] + insts["WRITE_SIZE"].get(k, 0.0)
                                                                       for k in insts["FETCH_SIZE"]}} if family else {}),
                           "method": "rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE, separate passes over " + (os.path.relpath(child[0], ROOT) + " (one forward, same shapes)" if child else "tools/pmc_f5_eval.py (one DiT evaluation, same shapes)") +
                                     "; FETCH_SIZE x2 per the gfx950 note of MI355X_MICROARCH.md; "
                                     "fabric-side bytes (Infinity-Cache hits are counted)"}



def measure_f5_plus_bigvgan(torch, fb, f5_dtype: str, voc_dtype: str, U: int, steps: int, warmup: int):
    """The pipeline BASELINE.json's metric names — F5-TTS NFE=32 + BigVGAN-v2 24 kHz: preprocess -> 31 DiT evaluations with
    CFG -> the generated mel frames handed to the BigVGAN engine (mi_f5_synthesize_mel -> mi_bigvgan_forward) -> int16, all
    on the device.  (The reference's exported F5 graphs decode with Vocos — that is the headline line; this block is the
    same sampler with the BigVGAN vocoder of configs[0]/[1] behind it.)"""
    from mi355tts.config import BigVGANConfig
    from mi355tts.f5 import F5Engine
    from mi355tts.bigvgan import BigVGANVocoder
    import dataclasses
    dev, W = fb.dev, fb.W
    # the prompt features of the F5 *_bigvgan checkpoints: the bigvgan-type mel front end (modeling_modified/F5/modules.py:30-72)
    cfg = dataclasses.replace(fb.cfg, mel_spec_type="bigvgan", **fb.cfg_over)
    vcfg = BigVGANConfig()
    eng = F5Engine(cfg, blob_device=fb.blob_t, dtype=f5_dtype, device=fb.local)
    voc = BigVGANVocoder(vcfg, blob=W.pack_bigvgan(vcfg, W.synth_state(W.bigvgan_spec(vcfg), 9527)), dtype=voc_dtype, device=fb.local)
    audio, ids, N, noise = W.f5_synthetic_inputs(cfg, U, fb.rank, L=fb.L)
    R = cfg.ref_frames(audio.shape[1])
    F = N - R
    t_audio, t_ids, t_noise = torch.from_numpy(audio).to(dev), torch.from_numpy(ids).to(dev), torch.from_numpy(noise).to(dev)
    mel = torch.empty((U, cfg.mel_dim, F), dtype=torch.float32, device=dev)
    out = torch.empty((U, 1, voc.out_len(F)), dtype=torch.int16, device=dev)

    def step():
        eng.synthesize_mel_torch(t_audio, t_ids, N, noise=t_noise, out=mel)
        voc.run_torch(mel, out)

    for _ in range(max(warmup, 2)):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    tv = time.perf_counter()
    for _ in range(steps):
        voc.run_torch(mel, out)
    torch.cuda.synchronize()
    voc_ms = (time.perf_counter() - tv) / steps * 1e3
    audio_s = U * out.shape[-1] / vcfg.sampling_rate
    eng.close(); voc.close()
    return {"value": audio_s / dt, "unit": "audio-s/s", "ms_per_step": dt * 1e3, "rtf": dt / audio_s, "dtype": f"{f5_dtype} DiT + {voc_dtype} vocoder",
            "vocoder_ms_per_step": voc_ms, "mel_frames": F, "utterances_per_gpu": U,
            "mel_spec_type": cfg.mel_spec_type,
            "workload": f"F5-TTS {f5_dtype} NFE=32 (N={N}, bigvgan-type prompt mel: slaney basis, center=False, {R} prompt frames) -> generated mel "
                        f"({U},100,{F}) -> BigVGAN-v2 24khz_100band_256x {voc_dtype} -> int16, one device-resident pipeline "
                        f"(mi_f5_synthesize_mel + mi_bigvgan_forward)"}


def measure_f5_two_requests(torch, fb, dtype: str, steps: int, warmup: int):
    """Two single-utterance requests served CONCURRENTLY: two engine handles (two HIP streams, each replaying its own hipGraph) driven
    from two host threads — the serving form of configs[2].  The launch tails and gaps of one persistent-kernel chain are filled by
    the other (LOG.md round 4).  Not the headline (that is one utterance at a time): a secondary block."""
    import dataclasses
    import threading
    from mi355tts.f5 import F5Engine
    cfg = dataclasses.replace(fb.cfg, **fb.cfg_over)
    dev, W = fb.dev, fb.W
    engs = [F5Engine(cfg, blob_device=fb.blob_t, dtype=dtype, device=fb.local) for _ in range(2)]
    ins, outs = [], []
    for i in range(2):
        audio, ids, N, noise = W.f5_synthetic_inputs(cfg, 1, fb.rank, L=fb.L, first=i)
        R = cfg.ref_frames(audio.shape[1])
        ins.append((torch.from_numpy(audio).to(dev), torch.from_numpy(ids).to(dev), torch.from_numpy(noise).to(dev)))
        outs.append(torch.empty((1, 1, (N - R - 1) * cfg.hop_length), dtype=torch.int16, device=dev))

    def run(i, n):
        for _ in range(n):
            engs[i].synthesize_torch(ins[i][0], ins[i][1], N, noise=ins[i][2], out=outs[i])

    for i in range(2):
        run(i, max(warmup, 2))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    th = [threading.Thread(target=run, args=(i, steps)) for i in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    audio_s = 2 * outs[0].shape[-1] / cfg.sample_rate
    for e in engs:
        e.close()
    return {"value": audio_s / dt, "unit": "audio-s/s", "ms_per_round_of_two": dt * 1e3, "ms_per_utterance": dt * 5e2, "rtf": dt / audio_s, "dtype": dtype,
            "workload": f"two concurrent F5-TTS {dtype} NFE=32 requests (one utterance each, N={N}) on two engine handles / HIP streams of one GPU"}



def measure_f5_facade(torch, fb, dtype: str, steps: int, warmup: int):
    """The drop-in call shape itself (VERDICT r4 missing #3): the body of F5-TTS-ONNX-Inference.py:246-312 — ort_session_A.run, the
    31-call loop over ort_session_B, ort_session_C.run — through `import mi355tts.ort_compat as onnxruntime`, in both forms the
    driver has: the io-binding branch (:256-288, device-resident OrtValues, outputs bound onto inputs) and the plain
    `ort_session_B.run` branch (:290-304, host numpy in and out of every call).  Host int16 audio in, host int16 waveform out."""
    import dataclasses
    import tempfile
    from mi355tts import ort_compat as onnxruntime
    from mi355tts.f5 import F5Engine
    cfg = dataclasses.replace(fb.cfg, **fb.cfg_over)
    eng = F5Engine(cfg, blob_device=fb.blob_t, dtype=dtype, device=fb.local)
    audio, ids, N, _ = fb.W.f5_synthetic_inputs(cfg, 1, fb.rank, L=fb.L)
    audio = audio.reshape(1, 1, -1)
    text_ids = ids.reshape(1, -1)
    max_duration = np.array([N], dtype=np.int64)
    with tempfile.TemporaryDirectory(prefix="mi355tts_facade_") as td:
        wfile = os.path.join(td, "weights_in_hbm.npy")            # never read: the engine above is registered for it
        onnxruntime.register_engine("f5", cfg, wfile, dtype, fb.local, eng)
        sess = [onnxruntime.InferenceSession(onnxruntime.save_model(os.path.join(td, f"{k}.mi355.json"), k, cfg, wfile, dtype))
                for k in ("F5_Preprocess", "F5_Transformer", "F5_Decode")]
    ort_session_A, ort_session_B, ort_session_C = sess
    in_A, out_A = [a.name for a in ort_session_A.get_inputs()], [a.name for a in ort_session_A.get_outputs()]
    in_name_B, out_name_B = ort_session_B.get_inputs(), ort_session_B.get_outputs()
    in_C, out_C = [a.name for a in ort_session_C.get_inputs()], [a.name for a in ort_session_C.get_outputs()]
    NFE_STEP, FUSE_NFE, DEVICE_ID = cfg.nfe_step, max(1, cfg.fuse_step), fb.local

    def body(device_type):
        time_step = np.array([0], dtype=np.int32)
        noise, rope_cos_q, rope_sin_q, rope_cos_k, rope_sin_k, cat_mel_text, cat_mel_text_drop, ref_signal_len = ort_session_A.run(
            out_A, {in_A[0]: audio, in_A[1]: text_ids, in_A[2]: max_duration})
        if device_type:
            inputs = [onnxruntime.OrtValue.ortvalue_from_numpy(x, device_type, DEVICE_ID)
                      for x in (noise, rope_cos_q, rope_sin_q, rope_cos_k, rope_sin_k, cat_mel_text, cat_mel_text_drop, time_step)]
            outputs = [inputs[0], inputs[-1]]
            io_binding = ort_session_B.io_binding()
            for i in range(len(inputs)):
                io_binding.bind_ortvalue_input(name=in_name_B[i].name, ortvalue=inputs[i])
            for i in range(len(outputs)):
                io_binding.bind_ortvalue_output(name=out_name_B[i].name, ortvalue=outputs[i])
            for i in range(0, NFE_STEP - 1, FUSE_NFE):
                ort_session_B.run_with_iobinding(io_binding)
            noise = onnxruntime.OrtValue.numpy(io_binding.get_outputs()[0])
        else:
            for i in range(0, NFE_STEP - 1, FUSE_NFE):
                noise, time_step = ort_session_B.run([out_name_B[0].name, out_name_B[1].name], {
                    in_name_B[0].name: noise, in_name_B[1].name: rope_cos_q, in_name_B[2].name: rope_sin_q, in_name_B[3].name: rope_cos_k,
                    in_name_B[4].name: rope_sin_k, in_name_B[5].name: cat_mel_text, in_name_B[6].name: cat_mel_text_drop,
                    in_name_B[7].name: time_step})
        return ort_session_C.run([out_C[0]], {in_C[0]: noise, in_C[1]: ref_signal_len})[0]

    res = {}
    for key, dt_ in (("io_binding", "cuda"), ("host_numpy", None)):
        for _ in range(max(warmup, 1)):
            wav = body(dt_)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            wav = body(dt_)
        res[key] = (time.perf_counter() - t0) / steps * 1e3
    audio_s = wav.shape[-1] / cfg.sample_rate
    eng.close()
    return {"value": audio_s / (res["io_binding"] * 1e-3), "unit": "audio-s/s", "ms_per_step": res["io_binding"],
            "ms_per_step_host_numpy_form": res["host_numpy"], "rtf": res["io_binding"] * 1e-3 / audio_s, "dtype": dtype,
            "workload": f"the reference driver's bracket (F5-TTS-ONNX-Inference.py:246-312) through mi355tts.ort_compat: graph A run, "
                        f"{(NFE_STEP - 1 + FUSE_NFE - 1) // FUSE_NFE} graph-B calls (ms_per_step: io-binding branch, device-resident OrtValues; "
                        f"ms_per_step_host_numpy_form: ort_session_B.run with host arrays), graph C run; N={N}, host int16 in / out"}


def run_indextts(args, world, rank, local, dev, dist, torch):
    """BASELINE configs[4] minus graph A: one sentence = GPT-2 prompt pass + greedy mel-code decode (graphs B/C/D/E and
    the loop, Inference_IndexTTS_ONNX.py:723-783) + the speaker-conditioned BigVGAN (graph F, :787).  conds_latent and
    the vocoder conditioning vectors (graph A's outputs) are synthetic."""
    from mi355tts.config import IndexGPTConfig, BigVGANConfig
    from mi355tts import weights as W
    from mi355tts import _lib
    from mi355tts.indextts import IndexGPT
    from mi355tts.bigvgan import BigVGANVocoder
    gcfg, vcfg = IndexGPTConfig(), BigVGANConfig.indextts()
    gspec, vspec = W.gpt_spec(gcfg), W.bigvgan_spec(vcfg)
    ng = sum(int(np.prod(sh)) for _, sh, _ in gspec)
    nv = sum(int(np.prod(sh)) for _, sh, _ in vspec)
    graw = None
    if rank == 0:
        graw = W.synth_state(gspec, 9527, fast=True)
        blob_t = torch.from_numpy(np.concatenate([W.pack_gpt(gcfg, graw),
                                                  W.pack_bigvgan(vcfg, W.synth_state(vspec, 9527, fast=True))])).to(dev)
    else:
        blob_t = torch.empty(ng + nv, dtype=torch.float32, device=dev)
    bcast_ms = 0.0
    if world > 1:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        blob_t = bcast_device_blob(torch, dist, blob_t)
        torch.cuda.synchronize()
        bcast_ms = (time.perf_counter() - t0) * 1e3
    NB = max(1, args.batch)
    gcfg.max_batch = NB
    gpt = IndexGPT(gcfg, blob_device=blob_t[:ng].contiguous(), dtype=args.dtype, device=local)
    voc = BigVGANVocoder(vcfg, blob_device=blob_t[ng:].contiguous(), dtype=args.dtype, device=local)
    del blob_t
    n_text, n_tok = 30, args.tokens
    text = (np.arange(n_text, dtype=np.int32) * 37 + 11 * rank) % (gcfg.text_tokens - 2) + 2
    # graph A (Inference_IndexTTS_ONNX.py:700-707): 6 s of int16 prompt audio -> conds_latent (the GPT prompt's first rows) and
    # the vocoder conditioning vectors; synthetic seeded weights like the other engines
    from mi355tts.config import IndexCondConfig
    from mi355tts.indextts import IndexCond
    ccfg = IndexCondConfig()
    cond_eng = IndexCond(ccfg, W.synth_state(W.cond_spec(ccfg), 9527, fast=True), device=local)
    tt = np.arange(144000) / 24000.0
    prompt_audio = np.clip(0.1 * 32767 * np.sin(2 * np.pi * 220.0 * tt) + W.synth_normal_fast(7 + rank, "prompt_audio", (144000,), std=500.0),
                           -32768, 32767).astype(np.int16)
    text_h = gpt.text_embed(text)
    mel_h, _ = gpt.mel_embed(gcfg.start_mel_token, 0)
    n_cond = ccfg.latents

    def graph_a():
        vc, lat = cond_eng.run(prompt_audio)
        vc = np.concatenate([vc[ccfg.voc_initial:], vc[:ccfg.voc_initial]])      # graph F's input order: the stage vectors, then the speaker embedding layer's
        pr, cl = gpt.concat(lat[None], text_h, mel_h)
        return torch.from_numpy(vc).to(dev), torch.from_numpy(pr[0]).to(dev), int(cl[0]), pr

    vconds, prompt, P, prompt_np = graph_a()
    toks = torch.zeros((n_tok,), dtype=torch.int32, device=dev)
    hid = torch.zeros((n_tok, gcfg.hidden), dtype=torch.float32, device=dev)
    ncond = vcfg.upsample_initial_channel + sum(vcfg.stage_channels(i) for i in range(vcfg.num_upsamples))
    assert ncond == cond_eng.ncond and gcfg.hidden == ccfg.model_dim
    wav = torch.empty((1, 1, (n_tok - 2) * vcfg.hop + 30), dtype=torch.int16, device=dev)
    audio_s = NB * wav.shape[-1] / vcfg.sampling_rate
    if NB > 1:      # NB sentences per step: different texts, one shared weight stream per decode step
        ps = []
        for b in range(NB):
            tb = (np.arange(n_text, dtype=np.int32) * 37 + 11 * rank + 101 * b) % (gcfg.text_tokens - 2) + 2
            ps.append(gpt.concat(prompt_np[:, :n_cond], gpt.text_embed(tb), mel_h)[0][0])
        prompts_cat = torch.from_numpy(np.concatenate(ps, axis=0)).to(dev)
        toks_b = torch.zeros((NB, n_tok), dtype=torch.int32, device=dev)
        hid_b = torch.zeros((NB, n_tok, gcfg.hidden), dtype=torch.float32, device=dev)

    state = {"vconds": vconds, "prompt": prompt}

    def gpt_leg():
        if NB == 1:
            n = gpt.generate_torch(state["prompt"], n_tok, toks, hid, stop_tokens=[])
            assert n == n_tok
        else:
            n = gpt.generate_batch_torch(prompts_cat, [P] * NB, [n_tok] * NB, toks_b, hid_b, stop_tokens=[])
            assert (n == n_tok).all()

    def step():
        # prompt audio -> graph A -> prompt rows + vocoder conditioning (once per utterance, as the driver does), then
        # stop_tokens=[]: a fixed amount of work per sentence (random weights never emit the stop code on cue)
        state["vconds"], state["prompt"], _, _ = graph_a()
        gpt_leg()
        for b in range(NB):
            voc.run_latent_torch(hid if NB == 1 else hid_b[b], state["vconds"], wav)

    for _ in range(max(args.warmup, 2)):
        step()

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier()
    dt = time.perf_counter() - t0
    if args.dump_outputs:          # what the step returns: mel codes and latents of every sentence, the waveform of the last one
        dump_outputs(args.dump_outputs, {(k if world == 1 else f"{k}_rank{rank}"): v.cpu().numpy() for k, v in
                                         (("mel_codes", toks if NB == 1 else toks_b), ("latent", hid if NB == 1 else hid_b), ("waveform", wav))})
    gpt_s = pg = pa = None
    if args.full:
        # GPT leg alone (same state), then the roofline leg: one eager pass with HIP events around every GEMV / GEMM launch
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        gpt_leg()
        torch.cuda.synchronize()
        gpt_s = time.perf_counter() - t1
        _lib.prof_reset()
        _lib.prof_enable(["conv_gemm", "attn"])
        gpt_leg()
        torch.cuda.synchronize()
        _lib.prof_enable(())
        pg, pa = _lib.prof_get("conv_gemm"), _lib.prof_get("attn")
    dt = max_over_ranks(torch, dist, world, dt, dev)
    if rank != 0:
        gpt.close(); voc.close(); cond_eng.close()
        return
    esz = 4 if args.dtype == "f32" else 2
    achieved = (pg["bytes"] / (pg["ms"] * 1e-3) / 1e9 if pg["ms"] > 0 else 0.0) if pg else None
    wbytes = (gcfg.layers * 12 * gcfg.hidden * gcfg.hidden + gcfg.mel_codes * gcfg.hidden) * esz
    line = {
        "metric": "audio_seconds_per_second", "value": world * audio_s * args.steps / dt, "unit": "audio-s/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": f"IndexTTS-1.5 {args.dtype}: GPT-2 (24 x 1280, 20 heads) prompt pass of {P} rows + greedy decode of "
                               f"{n_tok} mel codes + BigVGAN graph F, {NB} sentence(s) per GPU per step, 6 s of int16 prompt audio through graph A "
                               f"(Conformer / Perceiver / ECAPA) every step (BASELINE configs[4], all six graphs)",
                   "tokens": n_tok, "prompt_rows": P, "audio_seconds_per_step_per_gpu": audio_s,
                   "sentences_per_gpu": NB,
                   "rtf": dt / args.steps / audio_s, "gpt_leg_ms": gpt_s * 1e3 if gpt_s else None,
                   "decode_tokens_per_s": NB * n_tok / gpt_s if gpt_s else None,
                   "weight_bytes_streamed_per_token_GB": wbytes / 1e9,
                   "decode_weight_stream_GBps": wbytes * n_tok / gpt_s / 1e9 if gpt_s else None,
                   "weights": "synthetic seeded (510 M GPT + vocoder)", "weight_bcast_ms": bcast_ms},
        "roofline": {"bound": "hbm", "kernel": "gemv_kernel (decode-step linear layers: weights streamed once per token)",
                     "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                     "traffic": None, "launches_per_step": pg["launches"], "avg_launch_ms": pg["ms"] / max(pg["launches"], 1),
                     "family_ms_per_step": pg["ms"], "attn_ms_per_step": pa["ms"],
                     "note": "event-timed in a separate eager pass (the timed region replays a hipGraph per token); the "
                             "family also holds the prompt pass's 4 x 24 MFMA GEMM launches"} if pg else None,
    }
    if world == 1 and args.full and not args.no_cpu_baseline:
        from oracle import gpt_np as O
        n_cpu = 6
        folds = [O.fold_layer(gcfg, graw, i) for i in range(gcfg.layers)]
        keys = [np.zeros((gcfg.heads, 64, 0), np.float32)] * gcfg.layers
        vals = [np.zeros((gcfg.heads, 0, 64), np.float32)] * gcfg.layers
        pen = np.ones((1, gcfg.mel_codes), np.float32)
        t2 = time.perf_counter()
        keys, vals, kvl, last, tok, _ = O.graph_e(gcfg, graw, keys, vals, 0, pen, P, prompt_np, 1, folds)
        gl = np.array([1])
        for _ in range(n_cpu - 1):
            hs, gl = O.graph_c(gcfg, graw, tok, gl)
            keys, vals, kvl, last, tok, _ = O.graph_e(gcfg, graw, keys, vals, int(kvl[0]), pen, 1, hs, 0, folds)
        cpu_s = time.perf_counter() - t2
        line["cpu_baseline"] = {"value": n_cpu * vcfg.hop / vcfg.sampling_rate / cpu_s, "unit": "audio-s/s",
                                "cores": os.cpu_count(), "kind": "port",
                                "sample": f"numpy oracle, fp32: prompt pass of {P} rows + {n_cpu - 1} decode steps of the "
                                          f"same GPT (graph E only, no vocoder leg), {cpu_s:.1f} s; audio = tokens x 1024 / 24 kHz"}
    emit(line)
    gpt.close(); voc.close(); cond_eng.close()


def measure_bigvgan(torch, dist, world, rank, local, dev, dtype, B, F, steps, warmup, ixf, detail=True, keep_output=False):
    """BigVGAN-v2 (BASELINE configs[0]/[1]) or IndexTTS graph F (`ixf`): one step = one vocoder pass over the batch, mel
    resident in HBM.  Per-kernel HIP events are taken in a separate pass after the timed region (`detail`; a plain run skips
    it).  Returns (res, (cfg, state, the int16 waveform of the last timed step on the host if `keep_output`, else None))."""
    from mi355tts.config import BigVGANConfig
    from mi355tts import weights as W
    from mi355tts import _lib
    from mi355tts.bigvgan import BigVGANVocoder
    cfg = BigVGANConfig.indextts() if ixf else BigVGANConfig()
    spec = W.bigvgan_spec(cfg)
    nparam = sum(int(np.prod(s)) for _, s, _ in spec)
    state = None
    if rank == 0:
        state = synth_state_threaded(W, spec, 9527)
        blob_t = torch.from_numpy(W.pack_bigvgan(cfg, state)).to(dev)
    else:
        blob_t = torch.empty(nparam, dtype=torch.float32, device=dev)
    bcast_ms = 0.0
    if world > 1:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        blob_t = bcast_device_blob(torch, dist, blob_t)
        torch.cuda.synchronize()
        bcast_ms = (time.perf_counter() - t0) * 1e3
    voc = BigVGANVocoder(cfg, blob_device=blob_t, dtype=dtype, device=local)
    del blob_t
    out = torch.empty((B, 1, voc.out_len(F)), dtype=torch.int16, device=dev)
    audio_s = B * voc.out_len(F) / cfg.sampling_rate
    if ixf:
        latent = torch.from_numpy(W.synth_normal(100 + rank, "latent", (F + 2, cfg.num_mels), std=1.5, mean=0.3)).to(dev)
        ncond = cfg.upsample_initial_channel + sum(cfg.stage_channels(i) for i in range(cfg.num_upsamples))
        conds = torch.from_numpy(W.synth_normal(100 + rank, "conds", (ncond,), std=0.2)).to(dev)
        step = lambda: voc.run_latent_torch(latent, conds, out)
    else:
        mel = torch.from_numpy(W.bigvgan_synthetic_mel(cfg, B, F, rank)).to(dev)
        step = lambda: voc.run_torch(mel, out)
    for _ in range(warmup):
        step()

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    barrier()
    dt = time.perf_counter() - t0
    last = out.cpu().numpy() if keep_output else None
    dt = max_over_ranks(torch, dist, world, dt, dev)
    kernels, psteps = [], 0
    if detail:
        # per-kernel durations: a separate pass after the timed region, with every launch on the engine's one stream — in the
        # timed region the AMP blocks of a stage run on side streams (bigvgan_streams), where a launch's event-to-event time
        # includes whatever ran beside it
        _lib.set_option("bigvgan_streams", 1)
        step()
        _lib.prof_reset()
        _lib.prof_enable(["conv_gemm", "aa_act", "conv_post"])
        psteps = min(steps, 5)
        for _ in range(psteps):
            step()
        torch.cuda.synchronize()
        _lib.prof_enable(())
        kernels = _lib.prof_kernels()
        _lib.set_option("bigvgan_streams", USER_OPTIONS.get("bigvgan_streams", 3))       # (what the caller asked for with --option, else the default)
    voc.close()
    esz = 4 if dtype == "f32" else 2
    alg = bigvgan_algorithmic_bytes(cfg, B, F, esz)
    # dominant kernel: the MFMA-bound implicit-GEMM of stages 0-2 when it leads, else the HBM-bound fused AA conv
    roof = None
    if kernels:
        lead = kernels[0]
        mfma_bound = lead["kernel"].startswith("conv_gemm")
        roof = dominant_kernel_roofline(
            kernels, psteps, (MFMA_F32_PEAK_TF if dtype == "f32" else MFMA_F16_PEAK_TF) if mfma_bound else HBM_PEAK_GBS,
            "mfma" if mfma_bound else "hbm",
            "HIP events on the engine's stream around every launch, one separate one-stream pass after the timed region (the "
            "timed region runs the AMP blocks of a stage on side streams); per-launch work = 2*M*N*K flops "
            "(implicit GEMM) / layer-granular algorithmic bytes (x + w + out [+ res])")
    res = {"value": world * audio_s * steps / dt, "ms_per_step": dt / steps * 1e3, "dtype": dtype,
           "rtf": dt / steps / audio_s, "batch_per_gpu": B, "frames": F, "audio_seconds_per_step_per_gpu": audio_s,
           "workload": (f"IndexTTS graph F (speaker-conditioned BigVGAN, 1024x) {dtype}, T_codes = {F + 2} (BASELINE configs[4] "
                        f"vocoder leg)") if ixf else
                       (f"BigVGAN-v2 24khz_100band_256x {dtype} vocoder, mel ({B},100,{F}) per GPU (BASELINE configs[1])"),
           "weight_bcast_ms": bcast_ms, "whole_forward_algorithmic_GB": alg / 1e9,
           "whole_forward_algorithmic_GBps": alg / (dt / steps) / 1e9,
           "whole_forward_frac_of_hbm_peak": alg / (dt / steps) / 1e9 / HBM_PEAK_GBS, "roofline": roof}
    return res, (cfg, state, last)


def bigvgan_pmc(res, dtype: str, B: int):
    """roofline.traffic of the vocoder block: fabric-side bytes per launch of its dominant kernel AND of the whole forward (one
    forward of the same mel shape under two separate --pmc passes, tools/pmc_bigvgan.py), next to the layer-granular algorithmic
    bytes — traffic above the algorithmic figure is re-reads, below it is what the fusion saved."""
    if not res.get("roofline"):
        return
    tb, detail = pmc_traffic(res["roofline"]["kernel"], dtype, B, child=[os.path.join(ROOT, "tools", "pmc_bigvgan.py"), dtype, str(B), "1"])
    res["roofline"]["traffic"] = tb
    res["roofline"]["traffic_detail"] = detail
    if isinstance(detail, dict) and detail.get("whole_command_bytes"):
        res["whole_forward_fabric_GB"] = detail["whole_command_bytes"] / 1e9
        res["whole_forward_fabric_over_algorithmic"] = detail["whole_command_bytes"] / 1e9 / res["whole_forward_algorithmic_GB"]




def f5_secondaries(torch, dist, fb, args, N, local, dev):
    """The secondary blocks of the default one-GPU F5 run (`fb`: bench.F5Bench holding the device blob): the configs[3] shard, the
    native-fp32-MFMA / four-utterance / two-request forms of configs[2], the drop-in façade loop, F5 + BigVGAN, configs[1]."""
    secondary = {}
    if not (args.dtype == "bf16" and args.batch == 8):
        r2, _ = fb.measure("bf16", 8, 10, 2)
        r2["workload"] = f5_workload_name("bf16", 8, N)
        secondary["f5_bf16_u8"] = r2
    if args.dtype == "f32":
        # the same fp32 workload with the linear layers on the native fp32 MFMA (v_mfma_f32_32x32x2_f32) instead of the
        # fp16-pair products: both pass the same fp32 parity gates; reported so that either can be taken as the fp32 number
        r3, _ = fb.measure("f32", args.batch, 5, 2, f32_arithmetic="native-fp32-mfma")
        r3["workload"] = f5_workload_name("f32", args.batch, N) + " — linear layers, attention and position convolution on the native fp32 MFMA (F5Config.f32_arithmetic = native-fp32-mfma)"
        secondary["f5_f32_native_mfma"] = r3
        if args.batch == 1:
            # the same fp32 arithmetic with four utterances per step (8 CFG rows): what one GPU serves when requests
            # can be batched — the fixed per-launch cost of the DiT linear layers is shared by four times the rows
            r4, _ = fb.measure("f32", 4, 3, 1)
            r4["workload"] = f5_workload_name("f32", 4, N)
            secondary["f5_f32_u4"] = r4
    if not fb.small:
        secondary["f5_plus_bigvgan"] = measure_f5_plus_bigvgan(torch, fb, args.dtype, "f16", args.batch, 3, 2)
        if args.dtype == "f32" and args.batch == 1:
            secondary["f5_f32_two_requests"] = measure_f5_two_requests(torch, fb, "f32", 4, 2)
            secondary["f5_f32_facade"] = measure_f5_facade(torch, fb, "f32", 3, 1)
    secondary["bigvgan_f16_b8"] = measure_bigvgan(torch, dist, 1, 0, local, dev, "f16", 8, 512, 10, 3, False)[0]
    if not args.no_pmc:
        bigvgan_pmc(secondary["bigvgan_f16_b8"], "f16", 8)
    return secondary


def run_other(args, world, rank, local, dev, dist, torch):
    """`bench.py --workload indextts | bigvgan | indextts_f`."""
    if args.workload == "indextts":
        args.steps = 3 if args.steps is None else args.steps
        args.warmup = 3 if args.warmup is None else args.warmup
        args.batch = 1 if args.batch is None else args.batch
        args.dtype = "f16" if args.dtype is None else args.dtype
        run_indextts(args, world, rank, local, dev, dist, torch)
        return
    ixf = args.workload == "indextts_f"        # BASELINE configs[4] vocoder leg: IndexTTS graph F, T_codes = 128
    args.steps = 20 if args.steps is None else args.steps
    args.warmup = 3 if args.warmup is None else args.warmup
    args.dtype = "f16" if args.dtype is None else args.dtype
    B, F = (1, 126) if ixf else (8 if args.batch is None else args.batch, args.frames)
    res, (cfg, state, last) = measure_bigvgan(torch, dist, world, rank, local, dev, args.dtype, B, F, args.steps, args.warmup, ixf,
                                              detail=args.full, keep_output=bool(args.dump_outputs))
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"waveform" if world == 1 else f"waveform_rank{rank}": last})
    if rank != 0:
        return
    line = {"metric": "audio_seconds_per_second", "value": res["value"], "unit": "audio-s/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": res["ms_per_step"], "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {k: v for k, v in res.items() if k not in ("value", "ms_per_step", "dtype", "roofline")},
            "roofline": res["roofline"]}
    line["config"]["weights"] = "synthetic seeded (112.4 M params)"
    if world == 1 and args.full and not args.no_pmc and not ixf:
        bigvgan_pmc(res, args.dtype, B)
        line["roofline"] = res["roofline"]
        for k in ("whole_forward_fabric_GB", "whole_forward_fabric_over_algorithmic"):
            if k in res:
                line["config"][k] = res[k]
    if world == 1 and args.full and not args.no_cpu_baseline and not ixf:
        line["cpu_baseline"] = cpu_baseline_bigvgan(cfg, state, args.cpu_frames)
    emit(line)
