#!/usr/bin/env python3
"""Which kernel does launch_conv_gemm pick?  A fixed list of mi_bench_conv_gemm cases, each run once (three warm launches + one
timed) with the library profiler on: one JSON line (case, kernel label, launches) per kernel label of a case.

    python tools/gemm_plan_census.py [--out census.jsonl]
    rocprofv3 --kernel-trace --output-format csv -d trace -- python tools/gemm_plan_census.py --out census.jsonl
    python tools/gemm_plan_census.py --merge census.jsonl trace --out gemm_plan_census.json

--merge adds the grid and the workgroup size of every dispatch from the trace of the SAME run (cases run in list order, so the
GEMM dispatches of the trace are cut by the census's launch counts) and writes the fixture form that tests/test_gemm_plan.py and
tests/test_gpu_gemm_plan.py read: per case its arguments and, per launch of ONE call, label, grid and block.
"""
import argparse
import csv
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "text-to-speech-tts-onnx_amd")]

# (dtype, B, T, Cin, N, taps[, options]): at default options on 256 CUs these reach every kernel kind the entry can reach at
# defaults; five kinds need an option (the register-staged 128x128 tile, the ring with a plain epilogue, the two stream-K forms,
# fp16 pairs without gconv_pairs.hip), set for that case alone.  What the entry cannot reach (QKV epilogue, AdaLN fold, lengths,
# groups, 16-bit in with fp32 out) is pinned by the model tests (profiles/r18/INDEX.md names them)
CASES = [
    ("f16", 1, 300, 64, 32, 7),           # direct 256x32
    ("f16", 1, 300, 64, 48, 3),           # direct 128x64
    ("f16", 1, 300, 192, 192, 7, {"gemm_use_dma": 0, "gemm_use_dma3": 0}),     # direct 128x128
    ("f16", 1, 1152, 1024, 1024, 1),      # 64x64 DMA with the LDS epilogue
    ("f16", 1, 4608, 1024, 1024, 1),      # DMA 128 two-buffer
    ("f16", 1, 2304, 1024, 1024, 1, {"gemm_small16_max": 0}),                 # DMA 128 four-stage ring
    ("f16", 1, 12800, 1024, 1024, 1),     # ph8, 200 tiles
    ("f16", 1, 18016, 1024, 1024, 1),     # the row split: 16384 + 1632 rows
    ("f16", 1, 8192, 1024, 3072, 1, {"gemm_sk": 2, "gemm_ph8": 0}),           # 16-bit stream-K
    ("f16", 8, 5120, 128, 192, 7),        # dma3 at 192
    ("f16", 8, 2560, 512, 512, 7),        # dma3 at 256
    ("f16", 8, 5120, 512, 128, 7),        # dma3 at 128
    ("f16", 1, 512, 512, 384, 7),         # few tiles: still dma3 at 128
    ("f16", 1, 4608, 512, 1024, 7),       # falls through the dma3 tiles to DMA 128, direct epilogue
    ("bf16", 1, 12800, 1024, 1024, 1),    # the ladder differs by nothing but type
    ("f32", 1, 300, 64, 64, 3),           # the N = 64 kernel
    ("f32", 1, 300, 64, 64, 31, {"gemm_f32_gconv": 0}),                       # the N = 64 kernel with fp16 pairs (at the default
                                                                              # gconv_pairs.hip takes this shape before the plan is asked)
    ("f32", 1, 300, 256, 256, 1),         # f32 small 64x64
    ("f32", 1, 2252, 1024, 1024, 1),      # x3p (its exact-fit form)
    ("f32", 1, 2048, 1024, 1088, 1),      # x3
    ("f32", 1, 4096, 1024, 1088, 1, {"gemm_f32_x3": 0}),                      # f32 stream-K
    ("f32", 8, 4096, 128, 512, 3),        # f32 DMA 128
]
GEMM = re.compile(r"(conv_gemm_kernel|conv_gemm_dma_kernel|conv_gemm_dma3_kernel|linear_\w+_kernel|gconv\w*_kernel)")
CALLS = 4                                 # launch_conv_gemm calls per case: mi_bench_conv_gemm warms three times, then iters = 1


def census():
    import torch
    from mi355tts import _lib
    _lib.init(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _lib.prof_enable(("conv_gemm",))
    out = []
    for i, c in enumerate(CASES):
        opts = c[6] if len(c) > 6 else {}
        saved = {k: _lib.get_option(k) for k in opts}
        for k, v in opts.items():
            _lib.set_option(k, v)
        _lib.prof_reset()
        try:
            _lib.bench_conv_gemm(c[0], c[1], c[2], c[3], c[4], c[5], 1, iters=1)
        finally:
            for k, v in saved.items():
                _lib.set_option(k, v)
        ks = [k for k in _lib.prof_kernels() if GEMM.search(k["kernel"])]
        for k in sorted(ks, key=lambda k: k["kernel"]):
            out.append({"case": i, "args": list(c[:6]), "options": opts, "kernel": k["kernel"], "launches": k["launches"], "cus": cus})
    _lib.prof_enable(())
    return out


def merge(census_path, trace_dir):
    recs = [json.loads(l) for l in open(census_path)]
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if GEMM.search(r["Kernel_Name"]):
                wg = [int(r["Workgroup_Size_" + a]) for a in "XYZ"]
                rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"], [int(r["Grid_Size_" + a]) // w for a, w in zip("XYZ", wg)], wg))
    rows.sort()
    cases, at = [], 0
    for i, c in enumerate(CASES):
        mine = [r for r in recs if r["case"] == i]
        n = sum(r["launches"] for r in mine)
        assert n % CALLS == 0, (c, mine)
        per = n // CALLS                  # launches of one call (2: the row split)
        disp = rows[at:at + n]
        at += n
        assert len(disp) == n, f"the trace ends inside case {i}"
        for q in range(1, CALLS):         # every call of a case launches the same
            assert [d[1:] for d in disp[q * per:(q + 1) * per]] == [d[1:] for d in disp[:per]], (c, disp)
        labels = [r["kernel"] for r in mine]
        if per > 1:                       # order the labels as the launches ran: by the traced kernel's family name
            fam = [GEMM.search(d[1]).group(1) for d in disp[:per]]
            labels = [next(l for l in labels if f in l) for f in fam]
        assert len(labels) == per, (c, labels)
        cases.append({"args": list(c[:6]), "options": mine[0]["options"], "launches": [{"label": l, "grid": d[2], "block": d[3]} for l, d in zip(labels, disp[:per])]})
    assert at == len(rows), f"{len(rows) - at} GEMM dispatches of the trace belong to no case"
    return {"cus": recs[0]["cus"], "calls": CALLS, "cases": cases}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--merge", nargs=2, metavar=("CENSUS", "TRACE_DIR"))
    a = ap.parse_args()
    if a.merge:
        text = json.dumps(merge(*a.merge), indent=1) + "\n"
    else:
        text = "".join(json.dumps(r) + "\n" for r in census())
    if a.out:
        open(a.out, "w").write(text)
    sys.stdout.write(text)
