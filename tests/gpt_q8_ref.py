"""Float64 reference (TEST INFRASTRUCTURE) of the decode-step linears of the IndexTTS GPT on per-channel uint8 weights
(csrc/gpt_q8.hip), plain numpy, on top of tests/gpt_linear_ref.py.

    out = act(scale[n] * sum_k (q[n, k] - zp[n]) x'[k] + bias[n]) + res[n]

linear_q8() is gpt_linear_ref.linear on the float64 matrix (q - zp) * scale — the product of an integer of at most eight bits and a
float32 is exact in float64 — so its `mag` is scale[n] * sum_k |(q - zp) x'|, the scale of the tests' error bars.

The integer family (exact_case_q8): q any bytes and zp any byte, so (q - zp) is any integer in -255 .. 255; scale[n] a power of two
in 2^-3 .. 1; x integers in -4 .. 4; bias and res integers in -8 .. 8; no activation.  Every partial sum of every summation order
is an integer of magnitude at most 255 * 4 * K = 8 355 840 < 2^24 at K = 8192 (EXACT_SUM_MAX), a power-of-two scale moves only the
exponent, and scale * sum + bias + res spans at most bits 2^-3 .. 2^20: fp32 arithmetic is exact in any order, with or without a
fused multiply-add, and the result must equal the reference bit for bit (or its rounding, for a 16-bit output).

dequantized_state(cfg, state) is an upstream-named state whose fold (weights.fold_gpt, and the oracle's own fold_layer) gives the
dequantised blob of weights.gpt_q8_dequantized_blob: the four Conv1D kinds go back to (in, out), and the q / k rows of c_attn are
divided by head_dim^-0.25 in float64 before the one rounding to float32 — folding multiplies by it again in float32, so such a
weight comes back within one fp32 unit in the last place; every other weight comes back exactly.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

import gpt_linear_ref as R
from mi355tts import weights as W

K_EXACT_MAX = 8192
X_EXACT_MAX = 4
EXACT_SUM_MAX = 255 * X_EXACT_MAX * K_EXACT_MAX


def weights64(q, scale, zp):
    """(q - zp) * scale in float64: exact"""
    d = np.asarray(q, np.int64) - np.asarray(zp, np.int64)[:, None]
    return d.astype(np.float64) * np.asarray(scale, np.float32).astype(np.float64)[:, None]


def linear_q8(q, scale, zp, x, bias=None, res=None, act=False, ln=None, pre=None):
    return R.linear(weights64(q, scale, zp), x, bias, res, act, ln, pre)


def exact_case_q8(n, k, rows, *key, with_bias=True, with_res=True):
    """-> (q (n, k) uint8, scale (n) float32, zp (n) uint8, x (rows, k), bias (n) | None, res (rows, n) | None)"""
    assert k <= K_EXACT_MAX
    rng = np.random.default_rng([9527, 8, n, k, rows, *key])
    q = rng.integers(0, 256, (n, k)).astype(np.uint8)
    zp = rng.integers(0, 256, n).astype(np.uint8)
    zp[: min(n, 2)] = [0, 255][: min(n, 2)]
    q[0, : min(k, 4)] = [0, 255, 0, 255][: min(k, 4)]
    scale = (2.0 ** -rng.integers(0, 4, n)).astype(np.float32)
    x = rng.integers(-X_EXACT_MAX, X_EXACT_MAX + 1, (rows, k)).astype(np.float32)
    bias = rng.integers(-8, 9, n).astype(np.float32) if with_bias else None
    res = rng.integers(-8, 9, (rows, n)).astype(np.float32) if with_res else None
    return q, scale, zp, x, bias, res


def exact_sum_bound(k):
    """the largest magnitude a partial sum of the integer family can take at this K"""
    return 255 * X_EXACT_MAX * k


def dequantized_state(cfg, state):
    """upstream-named state whose fold is the dequantised blob (module docstring)"""
    st = OrderedDict((k, np.array(v, dtype=np.float32, copy=True)) for k, v in state.items())
    folded = W.fold_gpt(cfg, state)
    sc = np.float64(np.float32(float(cfg.head_dim) ** -0.25))
    h = cfg.hidden
    for name in st:
        if not name.endswith(W.GPT_Q8_KINDS):
            continue
        dq = W.dequantize_u8(*W.quantize_u8(folded[name]))              # (out, in) rows
        if name.endswith("lm_head.1.weight"):
            st[name] = dq
            continue
        d64 = dq.astype(np.float64)
        if name.endswith("attn.c_attn.weight"):
            d64[: 2 * h] /= sc
        st[name] = np.ascontiguousarray(d64.T).astype(np.float32)
    return st
