"""Float64 reference (TEST INFRASTRUCTURE) of the anti-aliased SnakeBeta kernels in 16-bit storage (csrc/aa_act.hip,
csrc/aa_conv.hip, csrc/aa_math.h), plain numpy, with the kernels' storage roundings written out and elementwise bounds.

Layout is the reference's: channels-first (B, C, T).  Everything is float64; a "16-bit value" is a float64 that q16 returns.

    q16(x, dtype)        x rounded to "f16" | "bf16", nearest even, straight from float64 (no float32 step in between)
    ulp16(x, dtype)      spacing of the type at |x|; below the smallest normal number the subnormal spacing (2^-24 | 2^-133)
    snake_params(alpha, beta, logscale)
                         (alpha, 1 / (beta + 1e-9)) as the float32 values make_snake (csrc/bigvgan.hip) uploads.  With
                         logscale=False they are exact; with logscale=True numpy's float32 exp stands in for expf
    activation1d(xq, alpha, beta, post=False, logscale=False)
                         Activation1d (act.py:25-29): zero-pad 5 (15), x2 transposed 12-tap kaiser-sinc filter, crop 15 / 15,
                         u + inv_beta sin^2(alpha u), zero-pad 5 / 6 (15 / 15), 12-tap filter stride 2.  post: T + 30 samples.
                         Filter: oracle.bigvgan_np.aa_filter(), the float32 taps
    activation1d_phase(...)  the same, and |alpha u| / (2 pi): the phase of every up-sampled sample in revolutions
    phase_term(phase, inv_beta, post, chain=None)   P of bound_act
    aa_conv(xq, alpha, beta, wq, bias, dilation, resq=None, *, dtype, logscale=False)
                         R_q = conv("same", q16(activation1d(xq)), wq) + bias + resq: the fused kernel's own rounding points
                         (input, activated tile, weights and residual in 16 bits), everything else exact
    bound_act(ref, P, dtype, A_act)            elementwise bound of the stand-alone kernel's 16-bit output against activation1d
    fused(xq, ..., dtype, A_act, A_conv=3e-5)  (R_q, bound_fused)

bound_act = 0.5 ulp16(ref) + A_act + P.  The first term is the output rounding.  A_act is the absolute term of the fp32
arithmetic and of v_sin_f32 (measured on the GPU, tests/test_gpu_aa_16bit.py).  P is what the fp32 rounding of the PHASE costs: the
kernel takes sin^2 of p = fl(fl(alpha / (2 pi)) * U) revolutions, d sin^2(2 pi p) / dp is at most 2 pi, and a relative error r of p
moves an up-sampled sample by at most inv_beta * 2 pi * |p| * r; the down filter carries it to the output as
    P[m] = sum_t |h[t]| * inv_beta * 2 pi * pmax[m] * 2^-22,      pmax[m] = max_t |p[2m - 5 + t]|  (the taps that feed output m).
The constant: r = 2^-22 = 4 u with u = 2^-24.  By the operation count of aa_math.h the phase product itself takes 2.7 u (the float32
1 / (2 pi) is 0.68 u off, alpha * s0 and al * U round once each) and the rest is the six-FMA chain of U, whose error is u times the
sum of its partial sums: at most 6 u * sum |tap x| / |U| in the worst case, about 1 u for partial sums of mixed sign.  The bound
keeps the 4 u; what a chain loses beyond it is part of A_act, which the GPU test caps at 1e-4.

bound_fused = 0.5 ulp16(R_q) + A_conv + conv(|wq|, ulp16(a_q) * mayflip).  a is the exact activation and a_q = q16(a).  An
activation the kernel computes within A_act + P of a lands on the same 16-bit value as a_q unless a lies that close to a rounding
boundary — mayflip = (q16(a - (A_act + P)) != q16(a + (A_act + P))) — and then it moves by one ulp16.  Where nothing flips the
kernel's products are the reference's, exact in fp32, and A_conv is the project's fp32 gate of this kernel for their fp32
accumulation (3e-5, tests/test_gpu_bigvgan.py test_fused_aa_conv_vs_oracle_f32).
"""
from __future__ import annotations

import numpy as np

from oracle import bigvgan_np as O

FORMATS = {"f16": (10, -14, 65504.0), "bf16": (7, -126, float(np.float32(3.3895313892515355e38)))}   # fraction bits, emin, largest
PHASE_REL = 2.0 ** -22
A_CONV = 3e-5


def _exponent(x, emin):
    """floor(log2 |x|), at least emin (exact: frexp)."""
    x = np.abs(np.asarray(x, np.float64))
    _, e = np.frexp(x)
    return np.where(x == 0, emin, np.maximum(e - 1, emin))


def ulp16(x, dtype):
    p, emin, _ = FORMATS[dtype]
    return np.ldexp(1.0, _exponent(x, emin) - p)


def q16(x, dtype):
    p, emin, big = FORMATS[dtype]
    x = np.asarray(x, np.float64)
    s = np.ldexp(1.0, _exponent(x, emin) - p)
    with np.errstate(invalid="ignore"):
        r = np.rint(x / s) * s                         # x / s is exact (a power of two); rint rounds half to even
    r = np.where(np.abs(r) > big, np.copysign(np.inf, x), r)
    return np.where(np.isfinite(x), r, x)


def snake_params(alpha, beta, logscale=False):
    a = np.asarray(alpha, np.float32)
    b = np.asarray(beta, np.float32)
    if logscale:
        a, b = np.exp(a).astype(np.float32), np.exp(b).astype(np.float32)
    ib = (np.float32(1.0) / (b + np.float32(1e-9))).astype(np.float32)
    return a.astype(np.float64), ib.astype(np.float64)


def _up(x, h, pad):
    """(u, chain): the up-sampled signal, and the sum of the magnitudes of the partial sums of each sample's six-term chain, taken in
    the kernel's order (aa_math.h: taps ascending, inputs descending) — u times it bounds the fp32 error of the kernel's U."""
    B, C, T = x.shape
    L = T + 2 * pad
    P = np.zeros((B, C, L))
    P[:, :, pad:pad + T] = x
    full = np.zeros((B, C, (L - 1) * 2 + 12))
    chain = np.zeros_like(full)
    for t in range(12):
        sl = slice(t, t + (L - 1) * 2 + 1, 2)
        full[:, :, sl] += h[t] * P
        chain[:, :, sl] += np.abs(full[:, :, sl])
    return 2.0 * full[:, :, 15:full.shape[2] - 15], 2.0 * chain[:, :, 15:chain.shape[2] - 15]


def _down_slices(s, pl, pr):
    """The 12 strided views of the zero-padded s that the down filter multiplies by h[0..11]."""
    B, C, n = s.shape
    Q = np.zeros((B, C, n + pl + pr))
    Q[:, :, pl:pl + n] = s
    To = (Q.shape[2] - 12) // 2 + 1
    return [Q[:, :, t:t + 2 * (To - 1) + 1:2] for t in range(12)]


def _pads(post):
    return (15, 15, 15) if post else (5, 5, 6)


def activation1d_phase(xq, alpha, beta, post=False, logscale=False, chain=False):
    """(y, phase) or, with chain=True, (y, phase, chain phase): alpha / (2 pi) times _up's chain."""
    h = O.aa_filter().astype(np.float64)
    al, ib = snake_params(alpha, beta, logscale)
    pad, pl, pr = _pads(post)
    u, ch = _up(np.asarray(xq, np.float64), h, pad)
    ph = al[None, :, None] * u
    s = u + ib[None, :, None] * np.sin(ph) ** 2
    y = sum(h[t] * v for t, v in enumerate(_down_slices(s, pl, pr)))
    phase = np.abs(ph) / (2.0 * np.pi)
    return (y, phase, al[None, :, None] * ch / (2.0 * np.pi)) if chain else (y, phase)


def activation1d(xq, alpha, beta, post=False, logscale=False):
    return activation1d_phase(xq, alpha, beta, post, logscale)[0]


def phase_term(phase, inv_beta, post=False, chain=None):
    """P of bound_act.  chain (activation1d_phase(..., chain=True)): the operation count in full instead of the flat 2^-22 —
    2.7 u of the phase for its product and u of the chain phase for U."""
    h = np.abs(O.aa_filter().astype(np.float64))
    _, pl, pr = _pads(post)
    err = phase * PHASE_REL if chain is None else (2.7 * phase + chain) * 2.0 ** -24
    return h.sum() * np.asarray(inv_beta, np.float64)[None, :, None] * 2.0 * np.pi * np.maximum.reduce(_down_slices(err, pl, pr))


def bound_act(ref, P, dtype, A_act):
    return 0.5 * ulp16(ref, dtype) + A_act + P


def conv_same(x, w, dilation):
    """x (B, Ci, T), w (Co, Ci, k), zero padding (k d - d) / 2 both sides, float64."""
    B, Ci, T = x.shape
    k = w.shape[2]
    pad = (k * dilation - dilation) // 2
    xp = np.zeros((B, Ci, T + 2 * pad))
    xp[:, :, pad:pad + T] = x
    out = np.zeros((B, w.shape[0], T))
    for j in range(k):
        out += np.einsum("oc,bct->bot", w[:, :, j], xp[:, :, j * dilation:j * dilation + T], optimize=True)
    return out


def aa_conv(xq, alpha, beta, wq, bias, dilation, resq=None, *, dtype, logscale=False):
    a = activation1d(xq, alpha, beta, False, logscale)
    out = conv_same(q16(a, dtype), np.asarray(wq, np.float64), dilation) + np.asarray(bias, np.float64)[None, :, None]
    return out if resq is None else out + np.asarray(resq, np.float64)


def fused(xq, alpha, beta, wq, bias, dilation, resq=None, *, dtype, A_act, A_conv=A_CONV, logscale=False):
    """(R_q, bound_fused)."""
    wq = np.asarray(wq, np.float64)
    a, phase = activation1d_phase(xq, alpha, beta, False, logscale)
    tol = A_act + phase_term(phase, snake_params(alpha, beta, logscale)[1])
    aq = q16(a, dtype)
    mayflip = q16(a - tol, dtype) != q16(a + tol, dtype)
    R = conv_same(aq, wq, dilation) + np.asarray(bias, np.float64)[None, :, None]
    if resq is not None:
        R = R + np.asarray(resq, np.float64)
    return R, 0.5 * ulp16(R, dtype) + A_conv + conv_same(ulp16(aq, dtype) * mayflip, np.abs(wq), dilation)


def rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, np.float64)))))
