"""CPU: the float64 reference of the GPT decode-step linears (tests/gpt_linear_ref.py) against the fp32 numpy oracle's layer
arithmetic (oracle/gpt_np.py) on one small layer, and the integer family's two promises by construction."""
from types import SimpleNamespace

import numpy as np

import gpt_linear_ref as R
from oracle import gpt_np as O

H, D = 2, 64
HID, INNER, S = H * D, 200, 12


def _layer():
    rng = np.random.default_rng(9527)
    p = "inference_model.transformer.h.0."
    st = {p + "attn.c_attn.weight": rng.normal(0, 0.05, (HID, 3 * HID)), p + "attn.c_attn.bias": rng.normal(0, 0.1, 3 * HID),
          p + "attn.c_proj.weight": rng.normal(0, 0.05, (HID, HID)), p + "attn.c_proj.bias": rng.normal(0, 0.1, HID),
          p + "ln_1.weight": 1 + rng.normal(0, 0.1, HID), p + "ln_1.bias": rng.normal(0, 0.1, HID),
          p + "ln_2.weight": 1 + rng.normal(0, 0.1, HID), p + "ln_2.bias": rng.normal(0, 0.1, HID),
          p + "mlp.c_fc.weight": rng.normal(0, 0.05, (HID, INNER)), p + "mlp.c_fc.bias": rng.normal(0, 0.1, INNER),
          p + "mlp.c_proj.weight": rng.normal(0, 0.05, (INNER, HID)), p + "mlp.c_proj.bias": rng.normal(0, 0.1, HID)}
    st = {k: np.asarray(v, np.float32) for k, v in st.items()}
    return SimpleNamespace(hidden=HID, heads=H, head_dim=D, layers=1, ln_eps=1e-5), st, p, rng


def _close(a, b, tol=2e-5):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape and np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max()), np.abs(a - b).max()


def test_mlp_half_matches_the_oracle():
    """ln_2 -> c_fc -> gelu_new, then c_proj + residual: graph E's lines for the MLP (oracle/gpt_np.py:112-114)"""
    cfg, st, p, rng = _layer()
    hs = rng.normal(0, 1, HID).astype(np.float32)
    m = O.gelu_new(O.layer_norm(hs, st[p + "ln_2.weight"], st[p + "ln_2.bias"]) @ st[p + "mlp.c_fc.weight"] + st[p + "mlp.c_fc.bias"])
    want = hs + (m @ st[p + "mlp.c_proj.weight"] + st[p + "mlp.c_proj.bias"])
    a = R.linear(st[p + "mlp.c_fc.weight"].T, hs, st[p + "mlp.c_fc.bias"], act=True, ln=(st[p + "ln_2.weight"], st[p + "ln_2.bias"]))
    _close(a["out"], m)
    b = R.linear(st[p + "mlp.c_proj.weight"].T, a["out"], st[p + "mlp.c_proj.bias"], res=hs)
    _close(b["out"], want)
    assert np.all(a["mag"] >= np.abs(a["v"] - st[p + "mlp.c_fc.bias"]) - 1e-12)


def test_head_with_leading_norm_matches_the_oracle():
    """ln_f -> final_norm -> lm_head (oracle/gpt_np.py:115-118); the ln_f row is last_hidden_state"""
    cfg, st, p, rng = _layer()
    hs = rng.normal(0, 2, HID).astype(np.float32)
    g1, b1, g2, b2 = st[p + "ln_1.weight"], st[p + "ln_1.bias"], st[p + "ln_2.weight"], st[p + "ln_2.bias"]
    w, bias = st[p + "mlp.c_fc.weight"].T, st[p + "mlp.c_fc.bias"]
    last = O.layer_norm(hs[None], g1, b1)
    want = O.layer_norm(last, g2, b2) @ w.T + bias
    got = R.linear(w, hs, bias, ln=(g2, b2), pre=(g1, b1))
    _close(got["pre_out"], last[0])
    _close(got["out"], want[0])


def test_qkv_split_matches_the_oracle():
    """the folded c_attn through linear() + qkv_split() against the oracle's per-head q / k / v (oracle/gpt_np.py:101-108)"""
    cfg, st, p, rng = _layer()
    f = O.fold_layer(cfg, st, 0)
    sc = np.float32(float(D) ** -0.25)
    w = st[p + "attn.c_attn.weight"].T.copy()
    b = st[p + "attn.c_attn.bias"].copy()
    w[:2 * HID] *= sc
    b[:2 * HID] *= sc
    hs = rng.normal(0, 1, HID).astype(np.float32)
    xn = O.layer_norm(hs[None, None], st[p + "ln_1.weight"], st[p + "ln_1.bias"])
    q = np.matmul(xn, f["wq"]) + f["bq"]                        # (H, 1, D)
    k = np.matmul(xn, f["wk"]) + f["bk"]
    v = np.matmul(xn, f["wv"]) + f["bv"]
    K0 = rng.normal(0, 1, (H, S, D))
    V0 = rng.normal(0, 1, (H, S, D))
    row = R.linear(w, hs, b, ln=(st[p + "ln_1.weight"], st[p + "ln_1.bias"]))["out"]
    for hist in (0, 5, S - 1, S):
        qo, K1, V1 = R.qkv_split(row, K0, V0, hist)
        _close(qo, q[:, 0].reshape(-1))
        changed = np.zeros((H, S, D), bool)
        if hist < S:
            changed[:, hist] = True
            _close(K1[:, hist], k[:, 0])
            _close(V1[:, hist], v[:, 0])
        assert np.array_equal(K1[~changed], K0[~changed]) and np.array_equal(V1[~changed], V0[~changed])
    assert R.cache_index(64 + 3, 7) == (1, 7, 3)


def test_integer_family_is_exact_by_construction():
    for n, k, rows in ((37, 8, 1), (5, R.K_EXACT_MAX, 3), (16, 1352, 64)):
        w, x, bias, res = R.exact_case(n, k, rows)
        for a in (w, x, bias, res):
            for dt in ("bf16", "f16"):
                assert np.array_equal(R.round_to(a, dt), a), "an input is not exact in " + dt
            assert np.array_equal(a, np.rint(a))
        assert np.abs(w).max() <= 4 and np.abs(x).max() <= 3 and np.abs(bias).max() <= 8 and np.abs(res).max() <= 8
        # the largest magnitude any partial sum of any order can reach: every product, then bias and residual
        worst = np.abs(x.astype(np.float64)) @ np.abs(w.astype(np.float64)).T + np.abs(bias) + np.abs(res)
        assert worst.max() <= 12 * k + 16 <= 61456 < 2 ** 24
        ref = R.linear(w, x, bias, res)["out"]
        assert np.array_equal(ref, np.rint(ref)) and np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
