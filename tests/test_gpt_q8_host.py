"""CPU: the per-channel uint8 weight format of the IndexTTS GPT (include/mi355tts.h, mi_gpt_create_q8) — the host quantiser
mi_gpt_quantize_u8 against its numpy twin weights.quantize_u8, the properties the format promises, and the test helpers of
tests/gpt_q8_ref.py.  No GPU call."""
import numpy as np
import pytest

import gpt_q8_ref as Q
from mi355tts import _lib
from mi355tts import weights as W
from mi355tts.config import IndexGPTConfig


def _c_quantize(w):
    w = np.ascontiguousarray(w, np.float32)
    n, k = w.shape
    q, scale, zp = np.zeros((n, k), np.uint8), np.zeros(n, np.float32), np.zeros(n, np.uint8)
    _lib.check(_lib.load().mi_gpt_quantize_u8(w.ctypes.data, n, k, q.ctypes.data, scale.ctypes.data, zp.ctypes.data),
               "mi_gpt_quantize_u8")
    return q, scale, zp


def _cases():
    rng = np.random.default_rng(9527)
    out = {}
    for k in (16, 128, 1280, 5120):
        w = rng.normal(0, 0.02, (9, k)).astype(np.float32)
        w[1] = np.abs(w[1]) + np.float32(0.01)             # all positive
        w[2] = -np.abs(w[2]) - np.float32(0.01)            # all negative
        w[3] = 0                                           # all zero
        w[4, k // 2] = 3.0                                 # one outlier
        w[5, ::2] = 0                                      # exact zeros among the values
        w[6] *= np.float32(1e-6)
        w[7] *= np.float32(1e4)
        out[f"k{k}"] = w
    out["n1"] = rng.normal(0, 0.05, (1, 48)).astype(np.float32)
    out["n1_k16"] = rng.normal(0, 0.05, (1, 16)).astype(np.float32)
    out["ties"] = (np.arange(-255, 257, dtype=np.float32).reshape(2, 256) * np.float32(0.5))      # w / scale lands on .5
    return out


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_c1_c_quantiser_equals_numpy_twin_and_keeps_the_formats_promises(name):
    w = CASES[name]
    q, scale, zp = W.quantize_u8(w)
    cq, cs, cz = _c_quantize(w)
    assert q.dtype == zp.dtype == np.uint8 and scale.dtype == np.float32
    assert np.array_equal(cq, q) and np.array_equal(cs.view(np.uint32), scale.view(np.uint32)) and np.array_equal(cz, zp)
    dq = W.dequantize_u8(q, scale, zp)
    assert dq.dtype == np.float32
    err = np.abs(w.astype(np.float64) - dq.astype(np.float64))
    assert (err <= 0.5 * scale.astype(np.float64)[:, None] * (1 + 2.0 ** -22)).all(), float((err / scale[:, None]).max())
    assert (dq[w == 0] == 0).all(), "a zero weight did not come back as zero"
    assert np.array_equal(dq, (q.astype(np.int32) - zp.astype(np.int32)[:, None]).astype(np.float32) * scale[:, None])
    if name.startswith("k"):
        assert zp[1] == 0 and zp[2] == 255, (zp[1], zp[2])
        assert scale[3] == 1 and zp[3] == 0 and not q[3].any()
        for r in (0, 4, 6, 7):
            assert q[r].min() == 0 and q[r].max() == 255, (r, q[r].min(), q[r].max())


def test_c1_bad_shapes_are_refused():
    L = _lib.load()
    w = np.zeros((2, 16), np.float32)
    q, s, z = np.zeros((2, 16), np.uint8), np.zeros(2, np.float32), np.zeros(2, np.uint8)
    for n, k in ((0, 16), (2, 0), (-1, 16)):
        assert L.mi_gpt_quantize_u8(w.ctypes.data, n, k, q.ctypes.data, s.ctypes.data, z.ctypes.data) == _lib.MI_EINVAL
        assert b"mi_gpt_quantize_u8" in L.mi_last_error()
    assert L.mi_gpt_quantize_u8(None, 2, 16, q.ctypes.data, s.ctypes.data, z.ctypes.data) == _lib.MI_EINVAL
    with pytest.raises(ValueError):
        W.quantize_u8(np.zeros(16, np.float32))
    assert L.mi_gpt_quantize_u8(w.ctypes.data, 2, 16, q.ctypes.data, s.ctypes.data, z.ctypes.data) == 0


def test_c2_fold_of_the_dequantized_state_is_the_dequantized_blob():
    cfg = IndexGPTConfig.small()
    state = W.synth_state(W.gpt_spec(cfg), 11)
    blob = W.gpt_q8_dequantized_blob(cfg, W.pack_gpt(cfg, state))
    assert blob.dtype == np.float32 and blob.shape == W.pack_gpt(cfg, state).shape
    back = W.pack_gpt(cfg, Q.dequantized_state(cfg, state))
    ulp = np.spacing(np.maximum(np.abs(blob), np.abs(back)))
    assert (np.abs(back.astype(np.float64) - blob.astype(np.float64)) <= ulp).all()
    # everything outside the six matrix kinds is untouched, and the matrices did change
    plain = W.pack_gpt(cfg, state)
    off = 0
    for name, shape, _ in W.gpt_spec(cfg):
        n = int(np.prod(shape))
        if name.endswith(W.GPT_Q8_KINDS):
            assert not np.array_equal(blob[off:off + n], plain[off:off + n]), name
            if not name.endswith("c_attn.weight"):
                assert np.array_equal(back[off:off + n], blob[off:off + n]), name
        else:
            assert np.array_equal(blob[off:off + n], plain[off:off + n]), name
        off += n


def test_c3_the_exact_familys_sums_stay_below_2_to_the_24():
    assert Q.EXACT_SUM_MAX == 8355840 < 2 ** 24 and Q.exact_sum_bound(Q.K_EXACT_MAX) == Q.EXACT_SUM_MAX
    q, scale, zp, x, bias, res = Q.exact_case_q8(5, Q.K_EXACT_MAX, 3)
    assert q.dtype == np.uint8 and zp.dtype == np.uint8 and np.abs(x).max() <= Q.X_EXACT_MAX
    assert q.min() == 0 and q.max() == 255 and zp[0] == 0 and zp[1] == 255
    d = q.astype(np.int64) - zp.astype(np.int64)[:, None]
    assert (np.abs(x.astype(np.int64)) @ np.abs(d).T).max() <= Q.EXACT_SUM_MAX          # the sum of magnitudes bounds every partial sum
    m, e = np.frexp(scale)
    assert (m == 0.5).all() and (scale <= 1).all() and (scale >= 0.125).all()
    ref = Q.linear_q8(q, scale, zp, x, bias, res)["out"]
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref), "the integer family's results are not exact in fp32"
    # integers in -255 .. 255 are exact in f16 and bf16 (the operand forms of the kernels)
    i = np.arange(-255, 256, dtype=np.float32)
    assert np.array_equal(Q.R.round_to(i, "f16"), i) and np.array_equal(Q.R.round_to(i, "bf16"), i)
