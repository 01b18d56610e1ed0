"""CPU: the float64 reference of the 16-bit anti-aliased activation kernels (tests/aa_ref64.py) against the float32 oracle and the
reference model's own vectors, its quantisers against numpy / torch, and its bounds against a model of the kernels — the float32
oracle with the kernels' rounding points — which they must admit, and against three wrong kernels, which they must refuse."""
import os

import numpy as np
import pytest
import torch

import aa_ref64 as R
from mi355tts import weights as W
from oracle import bigvgan_np as O

DTYPES = ["f16", "bf16"]


def _snake(C):
    return W.synth_normal(6, "a", (C,), std=0.3), W.synth_normal(7, "b", (C,), std=0.3)


@pytest.mark.parametrize("std", [1.5, 8.0])
@pytest.mark.parametrize("post", [False, True])
def test_reference_agrees_with_the_float32_oracle(std, post):
    """1e-5 is the project's fp32 gate for this operation (test_aa_vs_oracle_f32); measured 1.4e-6 at std 1.5, 8.5e-6 at std 8."""
    x = W.synth_normal(5, "aa48500", (1, 48, 500), std=std)
    a, b = _snake(48)
    r32 = O.activation1d(x, a, b, O.aa_filter(), post=post)
    r64 = R.activation1d(x, a, b, post=post, logscale=True)
    assert r64.dtype == np.float64 and r64.shape == r32.shape
    assert np.abs(r64 - r32).max() < 1e-5


def test_reference_agrees_with_the_reference_models_own_vectors(golden_dir):
    g = np.load(os.path.join(golden_dir, "bigvgan_small.npz"))
    y = R.activation1d(g["act_x"], g["act_alpha"], g["act_beta"], logscale=True)
    assert np.abs(y - g["act_y"]).max() < 1e-5
    yp = R.activation1d(g["post_x"], g["post_alpha"], g["post_beta"], post=True, logscale=True)
    assert yp.shape[-1] == g["post_x"].shape[-1] + 30
    assert np.abs(yp - g["post_y"]).max() < 1e-5


def _hard_values(dtype):
    p, emin, big = R.FORMATS[dtype]
    one = 2.0 ** -p                                               # spacing in [1, 2)
    sub = 2.0 ** (emin - p)                                       # smallest subnormal
    v = [0.0, 1.0, 1.0 + 0.5 * one, 1.0 + 1.5 * one, 1.0 + 0.5 * one + 2.0 ** -40, 1.0 + 1.5 * one - 2.0 ** -40,   # ties, near ties
         2.0 - 0.5 * one, 1.0 - 0.25 * one, 0.5 * sub, 1.5 * sub, 2.5 * sub, 0.5 * sub * (1 + 2.0 ** -30), 3 * sub,
         2.0 ** emin, 2.0 ** emin - 0.5 * sub, 2.0 ** emin * (1 - 2.0 ** -p), big, big * (1 - 2.0 ** -20), big + 0.25 * R.ulp16(big, dtype),
         1.0 / 3.0, np.pi, 1e-3, 300.7]
    if dtype == "f16":                                            # float32 steps of bf16's far range would double-round in torch's path
        v += [big + 0.5 * R.ulp16(big, dtype), big + 0.49 * R.ulp16(big, dtype), 1e6]
    v = np.array(v, np.float64)
    return np.concatenate([v, -v])


def test_q16_is_numpy_float16_and_torch_bfloat16():
    v = _hard_values("f16")
    with np.errstate(over="ignore"):
        want = v.astype(np.float16).astype(np.float64)
    np.testing.assert_array_equal(R.q16(v, "f16"), want)
    # torch rounds float32 -> bfloat16, so the comparison runs on values that float32 holds exactly (every one above but the near
    # ties, which are there for the float64 path: they must round away from the tie)
    v = _hard_values("bf16")
    exact = v.astype(np.float32).astype(np.float64) == v
    assert exact.sum() >= 28
    want = torch.from_numpy(v[exact].astype(np.float32)).to(torch.bfloat16).to(torch.float64).numpy()
    np.testing.assert_array_equal(R.q16(v[exact], "bf16"), want)
    one = 2.0 ** -7
    np.testing.assert_array_equal(R.q16(np.array([1.0 + 0.5 * one + 2.0 ** -40, 1.0 + 1.5 * one - 2.0 ** -40]), "bf16"), [1.0 + one, 1.0 + one])
    rng = np.random.default_rng(3)
    r = rng.standard_normal(4096) * np.exp(rng.uniform(-12, 10, 4096))
    np.testing.assert_array_equal(R.q16(r, "f16"), r.astype(np.float16).astype(np.float64))
    r32 = r.astype(np.float32)
    np.testing.assert_array_equal(R.q16(r32.astype(np.float64), "bf16"), torch.from_numpy(r32).to(torch.bfloat16).to(torch.float64).numpy())


@pytest.mark.parametrize("dtype", DTYPES)
def test_ulp16_is_the_spacing(dtype):
    p, emin, big = R.FORMATS[dtype]
    x = np.array([1.0, 1.5, 1.999, 2.0, 0.75, 2.0 ** emin, 2.0 ** emin * 0.9, 0.0, big, -3.0])
    want = np.array([2.0 ** -p, 2.0 ** -p, 2.0 ** -p, 2.0 ** (1 - p), 2.0 ** (-1 - p), 2.0 ** (emin - p), 2.0 ** (emin - p), 2.0 ** (emin - p),
                     R.ulp16(big, dtype), 2.0 ** (1 - p)])
    np.testing.assert_array_equal(R.ulp16(x, dtype), want)
    v = np.abs(_hard_values(dtype)[:8]) + 0.1
    q = R.q16(v, dtype)
    assert np.all(R.q16(q + R.ulp16(q, dtype), dtype) == q + R.ulp16(q, dtype))          # the next value of the type
    assert np.all(np.abs(q - v) <= 0.5 * R.ulp16(v, dtype))


# ---- the bounds against a model of the kernels: the float32 oracle with the same rounding points -----------------------------------
FUSED = [(96, 11, 5, 300, 1), (24, 3, 1, 600, 2), (48, 7, 3, 515, 1)]


def _fused_case(C, k, d, T, B, dtype):
    x = R.q16(W.synth_normal(5, f"ac{C}{T}", (B, C, T), std=1.5), dtype)
    a, b = _snake(C)
    w = R.q16(W.synth_normal(8, f"w{C}{k}", (C, C, k), std=1.0 / np.sqrt(C * k)), dtype)
    bias = W.synth_normal(9, "bias", (C,), std=0.1)
    res = R.q16(W.synth_normal(10, f"r{C}{T}", (B, C, T)), dtype)
    return x, a, b, w, bias, res


def _fused_model(x, a, b, w, bias, res, d, dtype, alpha_scale=1.0, dead_row=None):
    f = np.float32
    act = O.activation1d(x.astype(f), (a + np.log(alpha_scale)).astype(f), b, O.aa_filter())
    aq = R.q16(act, dtype)
    if dead_row is not None:
        aq[:, :, dead_row] = 0.0
    k = w.shape[2]
    o = O.conv1d(aq.astype(f), w.astype(f), bias, dilation=d, padding=(k * d - d) // 2) + res.astype(f)
    return R.q16(o, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,k,d,T,B", FUSED)
def test_fused_bound_admits_the_float32_oracle_with_the_kernels_rounding_points(C, k, d, T, B, dtype):
    """Measured: largest error / bound 0.73 .. 1.00 over these cases, rms(y - R_q) / rms(q16(R_q) - R_q) 1.000 .. 1.001.  The ratio's
    gate: float32 noise (1e-6) next to the output rounding (ulp / sqrt(12) >= 1.4e-4 at 1.0) adds nothing in quadrature; what raises
    it are activations that round the other way, one ulp16 each through weights of size 1 / sqrt(C k): 1.01 leaves them room and is
    far inside the GPU test's cap of 1.5."""
    x, a, b, w, bias, res = _fused_case(C, k, d, T, B, dtype)
    y = _fused_model(x, a, b, w, bias, res, d, dtype)
    for A_act in (2e-5, 1e-4):
        Rq, bound = R.fused(x, a, b, w, bias, d, res, dtype=dtype, A_act=A_act, logscale=True)
        np.testing.assert_array_equal(Rq, R.aa_conv(x, a, b, w, bias, d, res, dtype=dtype, logscale=True))
        err = np.abs(y - Rq)
        assert int((err > bound).sum()) == 0, (A_act, float((err / bound).max()))
    ratio = R.rms(y - Rq) / R.rms(R.q16(Rq, dtype) - Rq)
    assert 1.0 - 1e-9 <= ratio < 1.01, ratio


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("post", [False, True])
def test_activation_bound_admits_the_float32_oracle(dtype, post):
    """A_act = 1e-5: the fp32 gate of the operation."""
    x = R.q16(W.synth_normal(5, "aa48333", (1, 48, 333), std=1.5), dtype)
    a, b = _snake(48)
    ref, phase = R.activation1d_phase(x, a, b, post=post, logscale=True)
    P = R.phase_term(phase, R.snake_params(a, b, True)[1], post)
    assert P.shape == ref.shape and 0 < P.max() < 1e-4
    y = R.q16(O.activation1d(x.astype(np.float32), a, b, O.aa_filter(), post=post), dtype)
    assert int((np.abs(y - ref) > R.bound_act(ref, P, dtype, 1e-5)).sum()) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_bounds_refuse_a_dead_row_and_a_scaled_phase(dtype):
    """The bounds bite.  Fused: one activated row of 515 lost.  Activation: 1 / (2 pi) off in its fifth digit (0.15915 -> 0.15916,
    3.2e-5 relative) at phases of up to some hundred revolutions, where the same model with the right constant is inside."""
    C, k, d, T, B = 48, 7, 3, 515, 1
    x, a, b, w, bias, res = _fused_case(C, k, d, T, B, dtype)
    Rq, bound = R.fused(x, a, b, w, bias, d, res, dtype=dtype, A_act=1e-4, logscale=True)
    y = _fused_model(x, a, b, w, bias, res, d, dtype, dead_row=300)
    bad = np.abs(y - Rq) > bound
    assert bad.any() and set(np.nonzero(bad)[2]) <= set(range(300 - 9, 300 + 10))
    a100 = (a + np.log(100.0)).astype(np.float32)
    ref, phase = R.activation1d_phase(x, a100, b, logscale=True)
    assert 50 < phase.max() < 400
    bound = R.bound_act(ref, R.phase_term(phase, R.snake_params(a100, b, True)[1]), dtype, 1e-4)
    f = np.float32
    good = R.q16(R.activation1d(x, np.exp(a100), np.exp(b)), dtype)       # float64 model: float32 sin has no business at 100 revolutions
    assert int((np.abs(good - ref) > bound).sum()) == 0
    off = R.q16(R.activation1d(x, (np.exp(a100) * f(0.15916 / 0.15915494)).astype(f), np.exp(b)), dtype)
    assert (np.abs(off - ref) > bound).mean() > 0.01
