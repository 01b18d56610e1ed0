"""Float64 reference (TEST INFRASTRUCTURE) of the decode-step linear launches of the IndexTTS GPT (csrc/gpt.hip gemv_d_kernel,
gemv_b_kernel, gemm_skinny_kernel, gemm_skinny_wide_kernel), plain numpy.

    out = act(W x' + bias) + res        W (n, k); x (k) or (rows, k); bias (n); res like out
    x'  = x | LN(x) | LN(LN_pre(x))     LayerNorm over k, biased variance, eps 1e-5, gain and shift per column
    act = gelu_new, the tanh form       0.5 v (1 + tanh(sqrt(2 / pi) (v + 0.044715 v^3)))

linear() also returns mag = sum_k |W_nk x'_k| — the scale of the tests' error bars — the value v before the activation, and the
row of the leading LayerNorm.

The QKV form: columns [hidden, 3 hidden) of a row do not go to the output but to cache row `hist` of the slot's K (the first
hidden of them) and V (the rest), column c at [c // 64][hist][c % 64] of a [head][max_seq][64] cache — only when hist < max_seq.
qkv_split() applies that to copies of the caches and returns the q third.

The integer family (exact_case): W in -4 .. 4, x in -3 .. 3, bias and res in -8 .. 8, no activation.  Every input is exact in
bf16 (so in f16 and f32 too), and every partial sum of every summation order is an integer of magnitude at most
12 k + 16 <= 61456 < 2^24 for k <= 5120: fp32 accumulation is exact whatever its order, on v_dot2 and on the matrix cores, and the
result must equal the integer reference bit for bit.

round_to and ulp_bar are those of tests/gpt_attention_ref.py.
"""
from __future__ import annotations

import numpy as np

from gpt_attention_ref import round_to, ulp_bar          # noqa: F401  (re-exported for the tests)

EPS = 1e-5
K_EXACT_MAX = 5120


def layer_norm(x, gain, shift):
    x = np.asarray(x, np.float64)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + EPS) * np.asarray(gain, np.float64) + np.asarray(shift, np.float64)


def gelu_new(v):
    v = np.asarray(v, np.float64)
    return 0.5 * v * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (v + 0.044715 * v ** 3)))


def linear(w, x, bias=None, res=None, act=False, ln=None, pre=None):
    """-> dict: out, v (before the activation), mag (sum_k |w x'|), xp (x'), pre_out (LN_pre(x), or None)"""
    w = np.asarray(w, np.float64)
    xp = np.asarray(x, np.float64)
    pre_out = None
    if pre is not None:
        assert ln is not None
        pre_out = xp = layer_norm(xp, *pre)
    if ln is not None:
        xp = layer_norm(xp, *ln)
    v = xp @ w.T
    if bias is not None:
        v = v + np.asarray(bias, np.float64)
    out = gelu_new(v) if act else v
    if res is not None:
        out = out + np.asarray(res, np.float64)
    return {"out": out, "v": v, "mag": np.abs(xp) @ np.abs(w).T, "xp": xp, "pre_out": pre_out}


def cache_index(c, pos):
    """column c of a k or v row at position pos -> index into a [head][max_seq][64] cache"""
    return c // 64, pos, c % 64


def qkv_split(row, K, V, hist):
    """row (3 hidden) of ONE slot, K / V (heads, max_seq, 64) -> (q (hidden), K', V'): copies with row `hist` written"""
    row = np.asarray(row)
    hidden = row.shape[0] // 3
    assert row.shape == (3 * hidden,) and K.shape == V.shape == (hidden // 64, K.shape[1], 64)
    K, V = np.array(K, dtype=np.float64), np.array(V, dtype=np.float64)
    if hist < K.shape[1]:
        for c in range(hidden):
            K[cache_index(c, hist)] = row[hidden + c]
            V[cache_index(c, hist)] = row[2 * hidden + c]
    return row[:hidden].copy(), K, V


def exact_case(n, k, rows, *key, with_bias=True, with_res=True):
    """the integer family: (w (n, k), x (rows, k), bias (n) | None, res (rows, n) | None), float32 arrays of small integers"""
    assert k <= K_EXACT_MAX
    rng = np.random.default_rng([9527, n, k, rows, *key])
    w = rng.integers(-4, 5, (n, k)).astype(np.float32)
    x = rng.integers(-3, 4, (rows, k)).astype(np.float32)
    bias = rng.integers(-8, 9, n).astype(np.float32) if with_bias else None
    res = rng.integers(-8, 9, (rows, n)).astype(np.float32) if with_res else None
    return w, x, bias, res
