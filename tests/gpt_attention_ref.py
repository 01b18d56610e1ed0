"""Float64 reference (TEST INFRASTRUCTURE) of the four attention launches of the IndexTTS GPT (csrc/gpt_attn.h), plain numpy.

Layouts are the engine's: q (rows, heads * 64) — the q third of a qkv row, pre-scaled by the folded weights, so there is no
scale here — and K / V caches [slot][head][max_seq][64].

    decode(q, K, V, kv)                         row r = slot r: softmax over keys 0 .. kv[r]-1 of q.K, times V
    beam_gather(K, V, hist, ndec, beams, anc)   the private cache every hypothesis would own: position j < P from the group's
                                                first slot, position P + n from slot anc[ndec & 1][slot][n] of the group,
                                                P = hist - ndec + 1; decode() on it is the beam launch
    prompt(q, K, V, hist, rows, flag)           softmax(q.K + mask) V over keys 0 .. hist+rows-1 of ONE slot; mask = -128 * flag
                                                where j > i, j the absolute key index, i the row's index inside the new block
                                                (oracle/gpt_np.py:93-96) — added, not -inf, and no key is skipped
    prompt_packed(q, K, V, segs)                prompt() per segment (first, rows, slot) with history 0 and the mask on

Rows a launch must not read (>= kv, other slots' rows a table does not name) are never touched here either, so a test may
fill them with NaN.

round_to(x, dtype) is the rounding the tests apply to their inputs before either side sees them: to f32 / f16 / bf16, nearest
even, then every entry below 2^-14 in magnitude set to zero (nothing rests on subnormals); NaN stays NaN.  ulp_bar(ref, dtype)
is one unit in the last place of the output type at |ref|, as a relative bound: 2^-10 |ref| for f16, 2^-7 |ref| for bf16.
"""
from __future__ import annotations

import numpy as np

D = 64
MASK = -128.0


def _bf16_round(x32):
    b = np.ascontiguousarray(x32, np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16          # nearest, ties to even
    out = r.astype(np.uint32).view(np.float32)
    return np.where(np.isnan(x32), np.float32(np.nan), out).astype(np.float32)


def round_to(x, dtype):
    """x -> float32 array whose values are exact in `dtype` ("f32" | "f16" | "bf16"), |values| < 2^-14 flushed to 0."""
    x = np.asarray(x, np.float32)
    if dtype == "f16":
        with np.errstate(over="ignore"):
            x = x.astype(np.float16).astype(np.float32)
    elif dtype == "bf16":
        x = _bf16_round(x)
    elif dtype != "f32":
        raise ValueError(dtype)
    return np.where(np.abs(x) < 2.0 ** -14, np.float32(0), x).astype(np.float32)      # NaN compares false: kept


def ulp_bar(ref, dtype):
    return {"f32": 0.0, "f16": 2.0 ** -10, "bf16": 2.0 ** -7}[dtype] * np.abs(ref)


def _heads(q):
    q = np.asarray(q, np.float64)
    return q.reshape(q.shape[0], -1, D)                          # (rows, H, 64)


def _attend(qh, Kh, Vh, mask=None):
    """qh (64,), Kh / Vh (n, 64), mask (n,) or None -> (64,)"""
    s = Kh.astype(np.float64) @ qh
    if mask is not None:
        s = s + mask
    p = np.exp(s - s.max())
    return (p / p.sum()) @ Vh.astype(np.float64)


def decode(q, K, V, kv):
    qh = _heads(q)
    out = np.zeros(qh.shape, np.float64)
    for r in range(qh.shape[0]):
        n = int(kv[r])
        for h in range(qh.shape[1]):
            out[r, h] = _attend(qh[r, h], K[r, h, :n], V[r, h, :n])
    return out.reshape(qh.shape[0], -1)


def beam_gather(K, V, hist, ndec, beams, anc):
    """-> (Kp, Vp, kv): per-slot private caches (rows >= kv are NaN) and the key counts min(hist + 1, max_seq)"""
    K, V, anc = np.asarray(K), np.asarray(V), np.asarray(anc)
    ns, _, S, _ = K.shape
    Kp = np.full(K.shape, np.nan, K.dtype)
    Vp = np.full(V.shape, np.nan, V.dtype)
    kv = np.minimum(np.asarray(hist) + 1, S)
    for s in range(ns):
        s0 = s // beams * beams
        P = int(hist[s]) - int(ndec[s]) + 1
        tab = anc[int(ndec[s]) & 1, s]
        for j in range(int(kv[s])):
            src = s0 + (int(tab[j - P]) if j >= P else 0)
            Kp[s, :, j] = K[src, :, j]
            Vp[s, :, j] = V[src, :, j]
    return Kp, Vp, kv


def prompt(q, K, V, hist, rows, flag):
    """q (rows, hidden), K / V (heads, max_seq, 64) of one slot -> (rows, hidden)"""
    qh = _heads(q)
    n = int(hist) + int(rows)
    j = np.arange(n)
    out = np.zeros((rows, qh.shape[1], D), np.float64)
    for i in range(rows):
        mask = np.where(j > i, MASK, 0.0) * float(int(flag))
        for h in range(qh.shape[1]):
            out[i, h] = _attend(qh[i, h], K[h, :n], V[h, :n], mask)
    return out.reshape(rows, -1)


def prompt_packed(q, K, V, segs):
    """q (total, hidden), K / V (slots, heads, max_seq, 64), segs = [(first, rows, slot)] -> (total, hidden)"""
    q = np.asarray(q)
    out = np.zeros(q.shape, np.float64)
    for first, rows, slot in segs:
        out[first:first + rows] = prompt(q[first:first + rows], K[slot], V[slot], 0, rows, 1)
    return out
