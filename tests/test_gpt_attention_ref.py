"""CPU: the float64 attention reference of the GPU tests (tests/gpt_attention_ref.py) against the attention inside the GPT
oracle, oracle/gpt_np.graph_e — so that the reference the kernels are held to cannot itself be wrong about the mask's row
index, the key range or the missing scale.

graph_e exposes no attention output, so the model around it is made transparent: two layers with hand-made folds.  Layer 0
has random q / k / v projections, a c_proj that puts every head's 64 columns back in place and a zero MLP, so the hidden state
after it is hs + attention.  Layer 1 has an identity LayerNorm affine and a v projection that copies columns, so the value
rows graph_e returns for layer 1 are LayerNorm(hs + attention), every row of the new block.  The test rebuilds q, K, V and
that LayerNorm in float64 around gpt_attention_ref.prompt.

The oracle computes in float32; for the 1e-12 agreement its own code is run with float64 in place of float32 (the module's
`np.float32` swapped), and once more untouched at a float32 tolerance to show the swap changed nothing else.
"""
import types

import numpy as np
import pytest

import gpt_attention_ref as R
from oracle import gpt_np as G

H, DH, HID, INNER, CODES = 2, 64, 128, 16, 8
HIST, ROWS = 5, 7


class _Numpy64:
    """numpy with float32 spelled float64: what oracle/gpt_np.py sees as `np` in the float64 run"""
    float32 = np.float64

    def __getattr__(self, name):
        return getattr(np, name)


def _case():
    rng = np.random.default_rng(20)
    cfg = types.SimpleNamespace(layers=2, ln_eps=1e-5, heads=H, head_dim=DH, hidden=HID)
    st = {}
    for i in range(2):
        p = f"inference_model.transformer.h.{i}."
        st[p + "ln_1.weight"] = np.ones(HID) if i else rng.normal(1.0, 0.2, HID)
        st[p + "ln_1.bias"] = np.zeros(HID) if i else rng.normal(0.0, 0.2, HID)
        st[p + "ln_2.weight"] = np.ones(HID)
        st[p + "ln_2.bias"] = np.zeros(HID)
        st[p + "mlp.c_fc.weight"] = rng.normal(0, 0.1, (HID, INNER))
        st[p + "mlp.c_fc.bias"] = np.zeros(INNER)
        st[p + "mlp.c_proj.weight"] = np.zeros((INNER, HID))           # the MLP adds nothing
        st[p + "mlp.c_proj.bias"] = np.zeros(HID)
    st["inference_model.transformer.ln_f.weight"] = np.ones(HID)
    st["inference_model.transformer.ln_f.bias"] = np.zeros(HID)
    st["inference_model.lm_head.0.weight"] = np.ones(HID)
    st["inference_model.lm_head.0.bias"] = np.zeros(HID)
    st["inference_model.lm_head.1.weight"] = rng.normal(0, 0.1, (CODES, HID))
    st["inference_model.lm_head.1.bias"] = np.zeros(CODES)
    place = np.zeros((H, DH, HID))                                      # head h's column d -> hidden column h * 64 + d
    for h in range(H):
        place[h, np.arange(DH), h * DH + np.arange(DH)] = 1.0
    f0 = {"wq": rng.normal(0, 0.25, (H, HID, DH)), "bq": rng.normal(0, 0.1, (H, 1, DH)),
          "wk": rng.normal(0, 0.25, (H, HID, DH)), "bk": rng.normal(0, 0.1, (H, 1, DH)),
          "wv": rng.normal(0, 0.25, (H, HID, DH)), "bv": rng.normal(0, 0.1, (H, 1, DH)),
          "wo": place, "bo": np.zeros((1, 1, HID))}
    f1 = {"wq": np.zeros((H, HID, DH)), "bq": np.zeros((H, 1, DH)), "wk": np.zeros((H, HID, DH)), "bk": np.zeros((H, 1, DH)),
          "wv": place.transpose(0, 2, 1).copy(), "bv": np.zeros((H, 1, DH)), "wo": np.zeros((H, DH, HID)),
          "bo": np.zeros((1, 1, HID))}
    keys = [rng.normal(0, 1.5, (H, DH, HIST)), np.zeros((H, DH, HIST))]
    values = [rng.normal(0, 1.0, (H, HIST, DH)), np.zeros((H, HIST, DH))]
    hs = rng.normal(0, 1.0, (1, ROWS, HID))
    return cfg, st, [f0, f1], keys, values, hs


def _ln(x, w=1.0, b=0.0, eps=1e-5):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * w + b


def _expected(st, f0, keys, values, hs, flag):
    p = "inference_model.transformer.h.0."
    xn = _ln(hs[0], st[p + "ln_1.weight"], st[p + "ln_1.bias"])                       # (rows, hidden)
    q = np.concatenate([xn @ f0["wq"][h] + f0["bq"][h] for h in range(H)], axis=1)     # (rows, H * 64): the engine's q layout
    K = np.stack([np.concatenate([keys[0][h].T, xn @ f0["wk"][h] + f0["bk"][h]]) for h in range(H)])      # (H, kv, 64)
    V = np.stack([np.concatenate([values[0][h], xn @ f0["wv"][h] + f0["bv"][h]]) for h in range(H)])
    return _ln(hs[0] + R.prompt(q, K, V, HIST, ROWS, flag))


def _oracle(cfg, st, folds, keys, values, hs, flag):
    out = G.graph_e(cfg, st, keys, values, HIST, np.ones((1, CODES)), ROWS, hs, flag, folds)
    v1 = out[1][1]                                                                     # layer 1's values (H, hist + rows, 64)
    return np.asarray(v1)[:, HIST:].transpose(1, 0, 2).reshape(ROWS, HID)


@pytest.mark.parametrize("flag", [1, 0])
def test_reference_matches_the_oracle_attention(flag, monkeypatch):
    cfg, st, folds, keys, values, hs = _case()
    want = _expected(st, folds[0], keys, values, hs, flag)
    got32 = _oracle(cfg, st, folds, keys, values, hs, flag)
    assert np.abs(got32 - want).max() < 1e-4            # the oracle as it is: float32 LayerNorm and softmax, outputs of unit scale
    monkeypatch.setattr(G, "np", _Numpy64())
    got64 = _oracle(cfg, st, folds, keys, values, hs, flag)
    assert got64.dtype == np.float64
    err = float(np.abs(got64 - want).max())
    print(f"flag {flag}: max |reference - oracle in float64| = {err:.2e}")
    assert err < 1e-12


def test_the_case_can_tell_the_masks_apart():
    """history > 0 and an additive -128: mask on and off differ, and so does a mask whose row index is the absolute position"""
    cfg, st, folds, keys, values, hs = _case()
    on = _expected(st, folds[0], keys, values, hs, 1)
    off = _expected(st, folds[0], keys, values, hs, 0)
    assert np.abs(on - off).max() > 1e-2
    rng = np.random.default_rng(3)
    q = rng.normal(0, 1, (ROWS, HID))
    K = rng.normal(0, 1, (H, HIST + ROWS, DH))
    V = rng.normal(0, 1, (H, HIST + ROWS, DH))
    a = R.prompt(q, K, V, HIST, ROWS, 1)
    j = np.arange(HIST + ROWS)
    for i in range(ROWS):
        for h in range(H):
            s = K[h] @ q[i, h * DH:(h + 1) * DH] + np.where(j > i, -128.0, 0.0)
            w = np.exp(s - s.max())
            assert np.abs(a[i, h * DH:(h + 1) * DH] - (w / w.sum()) @ V[h]).max() < 1e-13
    shifted = np.stack([R.prompt(q[i:i + 1], K, V, HIST + i, 1, 0)[0] for i in range(ROWS)])      # keys 0 .. HIST + i, none masked
    assert np.abs(a - shifted).max() > 1e-2


def test_round_to():
    x = np.array([1.0, 1.0 + 2.0 ** -9, 1.0 + 2.0 ** -8 + 2.0 ** -9, 2.0 ** -15, -2.0 ** -14, 3.0e-6, np.nan], np.float32)
    b = R.round_to(x, "bf16")
    assert b[:3].tolist() == [1.0, 1.0, 1.0 + 2.0 ** -7] and b[3] == 0 and b[4] == -2.0 ** -14 and b[5] == 0 and np.isnan(b[6])
    h = R.round_to(x, "f16")
    assert h[:2].tolist() == [1.0, 1.0 + 2.0 ** -9] and h[3] == 0 and h[4] == -2.0 ** -14 and np.isnan(h[6])
    assert np.array_equal(R.round_to(h, "f16"), h, equal_nan=True)
    r = np.random.default_rng(0).normal(0, 1, 4096).astype(np.float32)
    import torch
    assert np.array_equal(R.round_to(r, "bf16"),
                          np.where(np.abs(r) < 2.0 ** -14, 0, torch.from_numpy(r).bfloat16().float().numpy()))
