"""GPU: the full-width DiT layers (dim 1024, 16 heads; two blocks, small front and back ends) against the float64 oracle
(tests/dit_oracle64.py) at every tiling the fp32 planner picks, and the 16-bit engines at the configs[3] batch shape.

A fp32 linear layer of the DiT goes either to the exact-fit kernel linear_x3d_kernel<TW, FOLD, EPK> (gemm_x3d.hip) or to the
stream-K panel-plane kernel linear_x3p_kernel (gemm_x3p.hip).  x3d_plan decides from the row count 2 U N and the layer width
(>= 90 % of the tiles' area useful), and picks the tile width (192 / 128 / 64) and band height.  The grid below reaches every
x3d instantiation that exists at dim 1024 — QKV (3072 columns) at 192, 128 and 64; FF1 (2048) and O / FF2 (1024) at 128 and 64,
in the AdaLN-fold and the row-norm form: 14 of the 18 compiled.  The other four (FF1 and O / FF2 at tile width 192, either form)
cannot be reached at this width: 192 divides neither 1024 nor 2048.  Each case names the kernels it must run, so that a planner
change shows up here instead of the grid quietly testing something else.

Every utterance of a batch is compared (pred[2u:2u+2]), by its overall rel RMS and by its worst single row: a fault confined to
one row group — the partial last one of N = 1037 (2074 rows: 58 of the last group's 144 are live) above all — hides in the
overall figure but not in the row one.
"""
import dataclasses

import numpy as np
import pytest

from mi355tts.config import F5Config
from mi355tts import weights as W
from mi355tts import _lib
from mi355tts.f5 import F5Engine
from oracle import f5_np as O

from dit_oracle64 import F32_OVERALL_GATE, F32_ROW_GATE, dit_errors, dit_forward64, rms, widen

pytestmark = pytest.mark.gpu

K_EVAL = 2          # grid index of the evaluation (t_emb = time_tables[2][K_EVAL])


def _mid_cfg(**kw):
    """test_gpu_f5._mid_cfg: full-width DiT layers, two blocks, small front / back end."""
    return F5Config(depth=2, text_dim=64, text_num_embeds=40, conv_layers=1, vocos_dim=64, vocos_intermediate=128, vocos_layers=1,
                    nfe_step=4, **kw)


def _inputs(cfg, U, N, seed=3):
    """test_gpu_f5._mid_inputs: utterance u depends on (N, u) alone, so references are shared between batch sizes."""
    noise = np.stack([W.synth_normal(seed + u, f"n{N}", (N, cfg.mel_dim)) for u in range(U)])
    cmt = np.stack([W.synth_normal(seed + 11 + u, f"c{N}", (N, cfg.mel_dim + cfg.text_dim), std=0.7) for u in range(U)])
    cmtd = np.stack([W.synth_normal(seed + 22 + u, f"d{N}", (N, cfg.mel_dim + cfg.text_dim), std=0.7) for u in range(U)])
    return noise, cmt, cmtd


@pytest.fixture(scope="module")
def mid():
    cfg = _mid_cfg()
    raw = W.synth_state(W.f5_spec(cfg), 7)
    st = W.fold_f5(cfg, raw)
    t_emb = O.time_tables(cfg, st)[2][K_EVAL]
    return cfg, raw, widen(st), t_emb, {}


def _refs(monkeypatch, mid, U, N):
    """float64 references of utterances 0 .. U-1 at N frames (computed once per (N, u) for the whole module)."""
    cfg, _, st64, t_emb, cache = mid
    noise, cmt, cmtd = _inputs(cfg, U, N)
    for u in range(U):
        if (N, u) not in cache:
            cache[(N, u)] = dit_forward64(monkeypatch, cfg, st64, noise[u], cmt[u], cmtd[u], t_emb)
    return (noise, cmt, cmtd), [cache[(N, u)] for u in range(U)]


def _eval_profiled(eng, noise, cmt, cmtd, families=("conv_gemm", "attn")):
    _lib.prof_reset(); _lib.prof_enable(families)
    try:
        a = eng.dit_eval(noise, cmt, cmtd, K_EVAL)
    finally:
        _lib.prof_enable(())
    return a, {k["kernel"]: k["launches"] for k in _lib.prof_kernels()}


@pytest.fixture(scope="module")
def f32_engines(mid):
    cfg, raw = mid[0], mid[1]
    e = {"fold": F5Engine(cfg, raw, dtype="f32"), "row-norm": F5Engine(dataclasses.replace(cfg, adaln_fold=False), raw, dtype="f32")}
    assert e["fold"].info()["adaln_fold"] and not e["row-norm"].info()["adaln_fold"]
    yield e
    for x in e.values():
        x.close()


@pytest.fixture(scope="module")
def seen():
    """kernel names per form, accumulated over the grid (test_every_reachable_x3d_instantiation_ran checks the union)."""
    return {"fold": set(), "row-norm": set()}


# x3d epilogue labels per layer role and form (gemm_x3d.hip launch_linear_x3d)
# ("in": the input projection, cat_ld() = 320 -> 1024 columns, a plain row-output layer in either engine)
ROLE = {"fold": {"QKV": "AdaLN fold, QKV", "FF1": "AdaLN fold, FF1", "O/FF2": "AdaLN fold, O / FF2", "in": "rows out"},
        "row-norm": {"QKV": "QKV", "FF1": "planes out", "O/FF2": "rows out", "in": "rows out"}}
X3P = {"fold": {"QKV": "AdaLN fold, QKV", "FF1": "AdaLN fold, FF1", "O/FF2": "AdaLN fold, O / FF2", "in": None},
       "row-norm": {"QKV": "QKV", "FF1": "planes out", "O/FF2": None, "in": None}}
ATTN_SLICED = "attn_x3f_kernel<false, pre-split K V, fp16 pairs> + key slices"
ATTN_WHOLE = "attn_x3f_kernel<false, pre-split K V, fp16 pairs>"


def x3d_label(tw, role, form):
    return f"linear_x3d_kernel<{tw}, {ROLE[form][role]}>"


def x3p_label(role, form):
    tail = X3P[form][role]
    return "linear_x3p_kernel<float, true, 2" + (f", {tail}>" if tail else ">")


# (U, N) -> tile width x3d_plan picks per DiT layer role (None: the stream-K kernel), and the attention tiling (unsliced from
# 1024 workgroups of 128 queries on: (N + 127) / 128 x 2 U x 16 heads)
GRID = {
    (1, 551): ({"QKV": None, "FF1": 64, "O/FF2": None, "in": None}, ATTN_SLICED),   # 1102 rows: FF1 alone, 8 row groups x 32 at TW 64
    (1, 701): ({"QKV": 128, "FF1": None, "O/FF2": None, "in": None}, ATTN_SLICED),  # 1402 rows: QKV, 10 x 24 at TW 128
    (1, 1036): ({"QKV": None, "FF1": None, "O/FF2": None, "in": None}, ATTN_SLICED),  # 2072 rows: 89.9 %, just below the window
    (1, 1037): ({"QKV": 192, "FF1": 128, "O/FF2": 64, "in": 64}, ATTN_SLICED),      # 2074 rows: the partial last row group (58 live rows)
    (1, 1152): ({"QKV": 192, "FF1": 128, "O/FF2": 64, "in": 64}, ATTN_SLICED),      # 16 whole row groups
    (1, 1153): ({"QKV": None, "FF1": None, "O/FF2": None, "in": None}, ATTN_SLICED),  # 17 row groups: back on stream-K
    (1, 1268): ({"QKV": None, "FF1": None, "O/FF2": None, "in": None}, ATTN_SLICED),  # the reference's own zh.wav prompt length
    (2, 1037): ({"QKV": 192, "FF1": 128, "O/FF2": 128, "in": 128}, ATTN_SLICED),    # two rounds, band 1; batch items split row groups
    (4, 1037): ({"QKV": 64, "FF1": 128, "O/FF2": 128, "in": 128}, ATTN_WHOLE),      # QKV at 48 column groups; 9 x 128 workgroups
    (4, 1126): ({"QKV": 192, "FF1": 128, "O/FF2": 128, "in": 128}, ATTN_WHOLE),     # four rounds (bench.py's u4 secondary)
}


# Achieved against the float64 oracle over the grid (both forms, every utterance): <= 1.24e-6 rel rms, <= 1.83e-6 worst row;
# the gates (tests/dit_oracle64.py) are 3.5e-6 and 5e-6
@pytest.mark.parametrize("U,N", list(GRID))
def test_fp32_dit_tiling_against_float64_oracle(monkeypatch, mid, f32_engines, seen, U, N):
    (noise, cmt, cmtd), refs = _refs(monkeypatch, mid, U, N)
    plan, attn = GRID[(U, N)]
    for form, eng in f32_engines.items():
        a, kernels = _eval_profiled(eng, noise, cmt, cmtd)
        seen[form] |= set(kernels)
        assert a.shape == (2 * U, N, mid[0].mel_dim) and np.isfinite(a).all()
        assert eng.info()["saturation_events"] == 0
        errs = [dit_errors(a[2 * u:2 * u + 2], refs[u]) for u in range(U)]
        e_all, e_row = max(e[0] for e in errs), max(e[1] for e in errs)
        print(f"fp32 {form:8s} U={U} N={N}: vs float64 oracle rel rms {e_all:.2e}, worst row {e_row:.2e} "
              f"(per utterance: {' '.join(f'{x:.2e}/{y:.2e}' for x, y in errs)})")
        print("   kernels: " + "; ".join(sorted(k for k in kernels if "linear_x3" in k or "attn" in k)))
        for role, tw in plan.items():
            if tw is not None:
                assert x3d_label(tw, role, form) in kernels, (form, U, N, role, tw, sorted(kernels))
            else:
                assert x3p_label(role, form) in kernels, (form, U, N, role, sorted(kernels))
        # nothing else on x3d: the planner took no layer the table does not name
        want = {x3d_label(tw, role, form) for role, tw in plan.items() if tw is not None}
        assert {k for k in kernels if "linear_x3d" in k} <= want, (form, U, N, sorted(kernels))
        other = ATTN_WHOLE if attn == ATTN_SLICED else ATTN_SLICED
        assert attn in kernels and other not in kernels, (form, U, N, sorted(kernels))
        for u, (ea, er) in enumerate(errs):
            assert ea < F32_OVERALL_GATE and er < F32_ROW_GATE, (form, U, N, u, ea, er)
        b = eng.dit_eval(noise, cmt, cmtd, K_EVAL)
        assert np.array_equal(a, b), (form, U, N)


def test_every_reachable_x3d_instantiation_ran(seen):
    """Across the grid: all 14 x3d instantiations reachable at dim 1024 (both forms), the stream-K kernels of each role and both
    attention tilings (runs after the grid; pytest keeps file order)."""
    assert seen["fold"] and seen["row-norm"], "the grid did not run"
    for form in ("fold", "row-norm"):
        want = {x3d_label(tw, role, form) for role, tws in (("QKV", (192, 128, 64)), ("FF1", (128, 64)), ("O/FF2", (128, 64)))
                for tw in tws}
        want |= {x3p_label(role, form) for role in ("QKV", "FF1", "O/FF2")} | {ATTN_SLICED, ATTN_WHOLE}
        assert want <= seen[form], (form, sorted(want - seen[form]))
        assert not any(k.startswith("linear_x3d_kernel<192, ") and "QKV" not in k for k in seen[form])


# ---------------------------------------------------------------------------------------------
# 16-bit engines at configs[3]'s batch shape (8 utterances) and at the odd 1037: every utterance against float64
# ---------------------------------------------------------------------------------------------
# achieved (both N, every utterance): f16 4.50e-4 rel rms / 5.97e-4 worst row, bf16 3.60e-3 / 4.77e-3; the overall gates are those of
# test_gpu_f5.test_adaln_fold_against_rownorm_path_and_oracle, the row gates 3x the achieved
@pytest.mark.parametrize("dtype,tol,row_tol", [("f16", 1.5e-3, 1.8e-3), ("bf16", 1.2e-2, 1.4e-2)])
@pytest.mark.parametrize("N", [1126, 1037])
def test_16bit_u8_against_float64_oracle(monkeypatch, mid, dtype, tol, row_tol, N):
    cfg, raw = mid[0], mid[1]
    U = 8
    (noise, cmt, cmtd), refs = _refs(monkeypatch, mid, U, N)
    eng = F5Engine(cfg, raw, dtype=dtype)
    try:
        a, kernels = _eval_profiled(eng, noise, cmt, cmtd)
        b = eng.dit_eval(noise, cmt, cmtd, K_EVAL)
    finally:
        eng.close()
    assert a.shape == (2 * U, N, cfg.mel_dim) and np.isfinite(a).all() and np.array_equal(a, b)
    errs = [dit_errors(a[2 * u:2 * u + 2], refs[u]) for u in range(U)]
    e_all, e_row = max(e[0] for e in errs), max(e[1] for e in errs)
    print(f"{dtype} U=8 N={N}: vs float64 oracle rel rms {e_all:.2e}, worst row {e_row:.2e}")
    print("   kernels: " + "; ".join(sorted(kernels)))
    T = {"f16": "_Float16", "bf16": "__bf16"}[dtype]
    want = {f"linear_ph8_kernel<{T}, {T}, false>", f"linear_ph8_kernel<{T}, float, false>", f"conv_gemm_dma_kernel<{T}, {T}, true, 2, 64>",
            f"conv_gemm_dma_kernel<{T}, float, false, 2, 64>", f"conv_gemm_dma_kernel<{T}, float, true, 2, 64>",
            f"conv_gemm_dma_kernel<{T}, float, true>", f"attn_kernel<{T}, false>"}
    want.add(f"conv_gemm_dma_kernel<{T}, {T}, true>" if N == 1126 else f"conv_gemm_dma_kernel<{T}, {T}, true, 4>")
    assert {k for k in kernels if k.startswith(("linear_", "conv_gemm_dma_kernel", "attn_"))} == want, sorted(kernels)
    for u, (ea, er) in enumerate(errs):
        assert ea < tol and er < row_tol, (dtype, N, u, ea, er)


# ---------------------------------------------------------------------------------------------
# the input projection's panel planes (K = cat_ld() = 320 > ff = 256 in F5Config.small()) once went into a buffer
# sized for K = ff; from ceil(rows / 128) x dim / 128 >= 64 tiles (2 U N >= 8065 rows) the split wrote past it
# ---------------------------------------------------------------------------------------------
def test_small_config_input_projection_on_panel_planes(monkeypatch):
    cfg = F5Config.small()
    raw = W.synth_state(W.f5_spec(cfg), 9527)
    st64 = widen(W.fold_f5(cfg, raw))
    t_emb = O.time_tables(cfg, W.fold_f5(cfg, raw))[2][K_EVAL]
    U, N = 4, 1100
    noise, cmt, cmtd = _inputs(cfg, U, N, seed=5)
    eng = F5Engine(cfg, raw, dtype="f32")
    try:
        a1, k1 = _eval_profiled(eng, noise[:1], cmt[:1], cmtd[:1], families=True)
        a, k4 = _eval_profiled(eng, noise, cmt, cmtd, families=True)
        b = eng.dit_eval(noise, cmt, cmtd, K_EVAL)
        info = eng.info()
    finally:
        eng.close()
    print("U=1: " + "; ".join(f"{k} x{n}" for k, n in sorted(k1.items())))
    print("U=4: " + "; ".join(f"{k} x{n}" for k, n in sorted(k4.items())))
    x3p = lambda ks: sum(n for k, n in ks.items() if k.startswith("linear_x3p_kernel"))
    assert np.isfinite(a).all() and np.array_equal(a, b) and info["saturation_events"] == 0
    # dim 128 runs the row form: the input projection and O, FF1, FF2 of each block through F5::gemm, whose rows are split into panel
    # planes; at U = 1 none of them has the 64 tiles the panel-plane kernel takes, at U = 4 (8800 rows, 69 x 1 tiles) all of them do
    assert x3p(k1) == 0 and x3p(k4) == 1 + 3 * cfg.depth, (k1, k4)
    for u in range(U):
        ref = dit_forward64(monkeypatch, cfg, st64, noise[u], cmt[u], cmtd[u], t_emb)
        ea, er = dit_errors(a[2 * u:2 * u + 2], ref)
        print(f"small fp32 U=4 N=1100 utterance {u}: vs float64 oracle rel rms {ea:.2e}, worst row {er:.2e}")
        assert ea < F32_OVERALL_GATE and er < F32_ROW_GATE, (u, ea, er)     # achieved <= 4.6e-7, worst row 1.9e-6
    assert rms(a[:2] - a1) / rms(a1) < 3e-6
