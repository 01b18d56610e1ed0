"""GPU: which attention kernel a (dtype, options, shape) launches — attention.hip attention_plan — one DiT evaluation per row of a
table, profiled like test_gpu_dit_tilings._eval_profiled.  Every row asserts the exact set of attn* profiler labels (recorded from
the launcher as it stood before the plan existed, so the table pins the dispatch), the result against oracle/f5_np.py at the gates
of the neighbouring tests, and equality with a second call.

Two models:
  * `small`: the reduced model of the attention tests (dim 256, 4 heads, depth 1).  Its layers are too narrow for the panel-plane
    GEMMs, so its fp32 evaluations take the ROWS form and attention gets K / V as plain rows or a transposed fp32 V — every form
    without "pre-split K V".  N = 63 is below the N >= 64 threshold of the 64-query split: the unsliced forms on a one-tile grid;
    N = 130 is three key stages, one key past a stage boundary.
  * `mid`: test_gpu_dit_tilings._mid_cfg() with one block (dim 1024, 16 heads) for the "pre-split K V" kernels, which run only in
    the FOLD / PLANES forms: the O projection needs 64 tiles of 128 x 128, i.e. 2 U N >= 897 rows — N = 449 for one utterance,
    N = 225 for the ragged pair, the smallest at which those forms run.  N = 449 is eight key stages, the last of one key.

Gates: fp32 atol 3e-4 (test_attention_against_oracle_ragged_lengths); f16 rel rms 1.5e-2 (test_attention_key_slices_agree); bf16 rel
rms 8e-2 (test_dit_16bit_ragged_batch_against_oracle, the same dim-256 model)."""
import dataclasses

import numpy as np
import pytest

from mi355tts import _lib
from mi355tts import weights as W
from mi355tts.config import F5Config
from mi355tts.f5 import F5Engine
from oracle import f5_np as O

pytestmark = pytest.mark.gpu

K_EVAL = 1
OPTIONS = ("attn_f32_x3", "attn_split", "attn_f32_planes", "attn_kv_planes")
RAGGED = {"small": (130, 67), "mid": (225, 67)}

PAIRS = "attn_x3f_kernel<{}, pre-split K V, fp16 pairs>"
BF16X3 = "attn_x3f_kernel<{}, pre-split K V>"


def _row(model, dtype, N, label, **opts):
    return pytest.param(model, dtype, N, opts, label, id="-".join([model, dtype, str(N)] + [f"{k[5:]}{v}" for k, v in opts.items()]))


# (model, engine, N | "ragged", options, the one attention label of the evaluation)
ROWS = [
    # fp32, both products split (attn_f32_x3 = 2, the default), K / V pre-split by the QKV epilogue: attn_split x attn_f32_planes
    _row("mid", "f32", 449, PAIRS.format("false") + " + key slices", attn_split=2, attn_f32_planes=2),
    _row("mid", "f32", 449, BF16X3.format("true"), attn_split=2, attn_f32_planes=3),       # three planes: back on the 64-query form
    _row("mid", "f32", 449, PAIRS.format("true"), attn_split=1, attn_f32_planes=2),
    _row("mid", "f32", 449, BF16X3.format("true"), attn_split=1, attn_f32_planes=3),
    _row("mid", "f32", 449, PAIRS.format("false"), attn_split=0, attn_f32_planes=2),
    _row("mid", "f32", 449, BF16X3.format("false"), attn_split=0, attn_f32_planes=3),
    # ... and K / V split by the kernel (attn_kv_planes = 0; the small model never pre-splits)
    _row("mid", "f32", 449, "attn_x3f_kernel<true>", attn_kv_planes=0),
    _row("mid", "f32", 449, "attn_x3f_kernel<false>", attn_kv_planes=0, attn_split=0),
    _row("small", "f32", 130, "attn_x3f_kernel<true>", attn_kv_planes=0),
    _row("small", "f32", 63, "attn_x3f_kernel<false>", attn_kv_planes=0),
    _row("small", "f32", 130, "attn_x3f_kernel<true>"),
    # fp32, q.k split / native
    _row("small", "f32", 130, "attn_kernel<float, true, x3>", attn_f32_x3=1),
    _row("small", "f32", 63, "attn_kernel<float, false, x3>", attn_f32_x3=1),
    _row("small", "f32", 130, "attn_kernel<float, true>", attn_f32_x3=0),
    _row("small", "f32", 63, "attn_kernel<float, false>", attn_f32_x3=0),
    # ragged batches: the VARLEN instantiation of each kernel family
    _row("mid", "f32", "ragged", PAIRS.format("false") + " + key slices + lengths"),
    _row("small", "f32", "ragged", "attn_x3f_kernel<true> + lengths"),
    _row("small", "f32", "ragged", "attn_kernel<float, true> + lengths", attn_f32_x3=0),
    _row("small", "f16", "ragged", "attn_kernel<_Float16, true> + lengths"),
    # 16-bit engines, split and unsplit
    _row("small", "f16", 130, "attn_kernel<_Float16, true>"),
    _row("small", "f16", 63, "attn_kernel<_Float16, false>"),
    _row("small", "bf16", 130, "attn_kernel<__bf16, true>"),
    _row("small", "bf16", 63, "attn_kernel<__bf16, false>"),
    # f16 with the reference's fp16 score rounding (score_scale != 1)
    _row("small", "f16-ref", 130, "attn_kernel<_Float16, true, reference-fp16 scores>"),
    _row("small", "f16-ref", 63, "attn_kernel<_Float16, false, reference-fp16 scores>"),
]


def _cfg(model):
    if model == "small":
        return F5Config(dim=256, depth=1, heads=4, dim_head=64, text_dim=64, text_num_embeds=40, conv_layers=1,
                        pos_conv_groups=4, vocos_dim=64, vocos_intermediate=128, vocos_layers=1, nfe_step=4)
    return F5Config(depth=1, text_dim=64, text_num_embeds=40, conv_layers=1, vocos_dim=64, vocos_intermediate=128, vocos_layers=1,
                    nfe_step=4)


def _inputs(cfg, N, seed=0):
    cd = cfg.mel_dim + cfg.text_dim
    return (W.synth_normal(3 + seed, f"n{N}", (N, cfg.mel_dim)), W.synth_normal(4 + seed, f"c{N}", (N, cd), std=0.7),
            W.synth_normal(5 + seed, f"d{N}", (N, cd), std=0.7))


@pytest.fixture(scope="module")
def models():
    """model -> (cfg, raw weights, oracle(N, seed)): float32 numpy references, computed once per (model, N, seed)"""
    out = {}
    for model in ("small", "mid"):
        cfg = _cfg(model)
        raw = W.synth_state(W.f5_spec(cfg), 7)
        st = W.fold_f5(cfg, raw)
        t_emb = O.time_tables(cfg, st)[2][K_EVAL]
        cache = {}

        def ref(N, seed=0, cfg=cfg, st=st, t_emb=t_emb, cache=cache):
            if (N, seed) not in cache:
                cos, sin = O.rope_tables(N, 64)
                cache[(N, seed)] = O.dit_forward(cfg, st, *_inputs(cfg, N, seed), t_emb, cos, sin)
            return cache[(N, seed)]
        out[model] = (cfg, raw, ref)
    return out


@pytest.fixture(scope="module")
def engines(models):
    """(model, engine kind) -> engine, created on first use"""
    made = {}

    def get(model, kind):
        if (model, kind) not in made:
            cfg, raw, _ = models[model]
            if kind == "f16-ref":
                cfg = dataclasses.replace(cfg, ref_fp16_attn=True)
            made[(model, kind)] = F5Engine(cfg, raw, dtype=kind.split("-")[0])
        return made[(model, kind)]
    yield get
    for e in made.values():
        e.close()


def _profiled(call):
    _lib.prof_reset(); _lib.prof_enable(("attn",))
    try:
        a = call()
    finally:
        _lib.prof_enable(())
    return a, {k["kernel"]: k["launches"] for k in _lib.prof_kernels()}


def _rms(x):
    return float(np.sqrt(np.mean(np.square(np.asarray(x, np.float64)))))


@pytest.mark.parametrize("model,kind,N,opts,label", ROWS)
def test_attention_dispatch(models, engines, model, kind, N, opts, label):
    cfg, _, oracle = models[model]
    eng = engines(model, kind)
    if N == "ragged":
        lengths = RAGGED[model]
        ins = [_inputs(cfg, n, seed=10 * u) for u, n in enumerate(lengths)]
        call = lambda: eng.dit_eval_ragged([i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins], K_EVAL)
        refs = [oracle(n, 10 * u) for u, n in enumerate(lengths)]
    else:
        x, c, d = _inputs(cfg, N)
        call = lambda: [eng.dit_eval(x[None], c[None], d[None], K_EVAL)]
        refs = [oracle(N)]
    saved = {k: _lib.get_option(k) for k in OPTIONS}
    try:
        for k, v in opts.items():
            _lib.set_option(k, v)
        a, kernels = _profiled(call)
        b = call()
    finally:
        for k, v in saved.items():
            _lib.set_option(k, v)
    attn = {k: n for k, n in kernels.items() if k.startswith("attn")}
    errs = [(float(np.abs(g - r).max()), _rms(g - r) / _rms(r)) for g, r in zip(a, refs)]
    print(f"{model} {kind} N={N} {opts}: {attn}; " + " ".join(f"max |err| {m:.2e} rel rms {r:.2e}" for m, r in errs))
    assert attn == {label: cfg.depth}, (sorted(attn), label)
    for g, r, g2 in zip(a, refs, b):
        assert g.shape == r.shape and np.isfinite(g).all()
        if kind == "f32":
            np.testing.assert_allclose(g, r, atol=3e-4)
        else:
            assert _rms(g - r) / _rms(r) < (8e-2 if kind == "bf16" else 1.5e-2)
        assert np.array_equal(g, g2)
    if kind == "f32":
        assert eng.info()["saturation_events"] == 0
