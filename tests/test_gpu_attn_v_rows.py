"""GPU: fp32 attention with V as rows — the QKV epilogue writes pre-split V as [bh][plane][key][64] like K, and attn_x3f_kernel
transposes it on its LDS reads (attention.hip VROWS) instead of the epilogue transposing it with 2-byte stores.

  * the default build against the numpy oracle at test_gpu_f5's attention gate (atol 3e-4), N = 67 (two stages, a last stage of
    three keys), 130 / 257 (one key past a stage boundary), 700 (key slices, uneven cuts), crossed with attn_split 1 / 2 (and 0:
    the unsliced 128-query form of large batches) and attn_f32_planes 2 / 3, plus one ragged batch per kernel form (the VARLEN instantiations);
  * bit identity with the V^T layout: the same cases in a child process with MI355TTS_ATTN_V_ROWS=0 (the switch is read once per
    process).  Both epilogue branches add the bias (or apply the folded LayerNorm) in the same order on the same staged values and
    split every value on its own, and the kernel's fragments hold the same keys in the same element order: EVERY element equal;
  * stale pad rows: N = 257 and then N = 67 on one engine == N = 67 on a fresh engine (rows 67 .. 127 of the V planes hold the
    longer evaluation's values).  What this proves is limited: those stale values are FINITE, and a masked key's probability is
    exactly 0, so a kernel that cleared nothing would pass too — it catches a stage that reads the wrong rows or lets a pad row
    reach a live key, not a missing clear.  Non-finite bytes cannot be planted there through the engine: every producer of the
    fp16-pair operands watches their range, and a NaN on the way to V switches the engine's arithmetic before it gets there.  That
    the clear does not depend on the buffer is by construction (attention.hip load_regs: by key row against NL, no load involved);
  * run to run: the same call three times.

The cases are evaluated once per process (`_evaluate_all`); this file is also the child's script."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "text-to-speech-tts-onnx_amd")
if __name__ == "__main__":
    for p in (ROOT, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)

from mi355tts import _lib
from mi355tts import weights as W
from mi355tts.config import F5Config
from mi355tts.f5 import F5Engine

pytestmark = pytest.mark.gpu

ATOL = 3e-4                          # tests/test_gpu_f5.py: test_attention_against_oracle_ragged_lengths
LENGTHS = (67, 130, 257, 700)
SPLITS = (1, 2)
PLANES = (2, 3)
RAGGED = (257, 67)                   # U = 2 of different lengths: utterance 1 ends inside the slab's second stage
K_EVAL = 1


def _cfg():
    """the reduced model of the neighbouring attention tests (tests/test_gpu_f5.py)"""
    return F5Config(dim=256, depth=1, heads=4, dim_head=64, text_dim=64, text_num_embeds=40, conv_layers=1,
                    pos_conv_groups=4, vocos_dim=64, vocos_intermediate=128, vocos_layers=1, nfe_step=4)


def _inputs(cfg, N, seed=0):
    cd = cfg.mel_dim + cfg.text_dim
    return (W.synth_normal(3 + seed, f"n{N}", (N, cfg.mel_dim)), W.synth_normal(4 + seed, f"c{N}", (N, cd), std=0.7),
            W.synth_normal(5 + seed, f"d{N}", (N, cd), std=0.7))


def _v_rows(eng):
    return int(_lib.load().mi_f5_info(eng._h, b"attn_v_rows"))


def _evaluate_all():
    """name -> DiT evaluation of every case, in this process's V layout; "v_rows" -> that layout."""
    cfg = _cfg()
    raw = W.synth_state(W.f5_spec(cfg), 7)
    out = {}
    saved = {k: _lib.get_option(k) for k in ("attn_split", "attn_f32_planes")}
    eng = F5Engine(cfg, raw, dtype="f32")
    try:
        out["v_rows"] = np.asarray(_v_rows(eng))
        for planes in PLANES:
            _lib.set_option("attn_f32_planes", planes)
            for split in SPLITS + (0,):
                _lib.set_option("attn_split", split)
                for N in (LENGTHS if split else (257,)):
                    x, c, d = _inputs(cfg, N)
                    out[f"p{planes}.s{split}.n{N}"] = eng.dit_eval(x[None], c[None], d[None], K_EVAL)
                # the VARLEN instantiation of this split's kernel form
                ins = [_inputs(cfg, N, seed=10 * u) for u, N in enumerate(RAGGED)]
                rag = eng.dit_eval_ragged([i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins], K_EVAL)
                for u in range(len(RAGGED)):
                    out[f"p{planes}.s{split}.ragged.u{u}"] = rag[u]
            _lib.set_option("attn_split", saved["attn_split"])
        out["saturation_events"] = np.asarray(eng.info()["saturation_events"])
    finally:
        for k, v in saved.items():
            _lib.set_option(k, v)
        eng.close()
    return out


if __name__ == "__main__":
    np.savez(sys.argv[1], **_evaluate_all())
    sys.exit(0)


from oracle import f5_np as O       # noqa: E402  (the child does not need the oracle)

CASES = [f"p{p}.s{s}.n{N}" for p in PLANES for s in SPLITS for N in LENGTHS] + [f"p{p}.s0.n257" for p in PLANES] + \
        [f"p{p}.s{s}.ragged.u{u}" for p in PLANES for s in SPLITS + (0,) for u in range(len(RAGGED))]


@pytest.fixture(scope="module")
def rows():
    got = _evaluate_all()
    assert int(got["v_rows"]) == 1, "the default layout of pre-split V is rows"
    assert int(got["saturation_events"]) == 0
    return got


@pytest.fixture(scope="module")
def transposed():
    """the same cases from a child process with the switch off"""
    env = dict(os.environ, MI355TTS_ATTN_V_ROWS="0")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "vt.npz")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        with np.load(path) as z:
            got = {k: z[k] for k in z.files}
    assert int(got["v_rows"]) == 0, "MI355TTS_ATTN_V_ROWS=0 selects the V^T layout"
    return got


@pytest.fixture(scope="module")
def oracle():
    """float32 numpy reference per (N, input seed), computed once"""
    cfg = _cfg()
    st = W.fold_f5(cfg, W.synth_state(W.f5_spec(cfg), 7))
    t_emb = O.time_tables(cfg, st)[2][K_EVAL]
    cache = {}

    def ref(N, seed=0):
        if (N, seed) not in cache:
            cos, sin = O.rope_tables(N, 64)
            cache[(N, seed)] = O.dit_forward(cfg, st, *_inputs(cfg, N, seed), t_emb, cos, sin)
        return cache[(N, seed)]
    return ref


def _ref_of(oracle, case):
    tail = case.split(".")[-1]
    if tail.startswith("u"):
        u = int(tail[1:])
        return oracle(RAGGED[u], 10 * u)
    return oracle(int(tail[1:]))


@pytest.mark.parametrize("case", CASES)
def test_v_rows_against_the_oracle(rows, oracle, case):
    ref = _ref_of(oracle, case)
    got = rows[case]
    assert got.shape == ref.shape and np.isfinite(got).all()
    print(f"{case}: max |err| {np.abs(got - ref).max():.2e} (gate {ATOL:.0e})")
    np.testing.assert_allclose(got, ref, atol=ATOL)


@pytest.mark.parametrize("case", CASES)
def test_v_rows_bit_identical_to_the_transposed_layout(rows, transposed, case):
    a, b = rows[case], transposed[case]
    assert a.shape == b.shape
    print(f"{case}: elements that differ {int((a != b).sum())}, max |diff| {np.abs(a - b).max():.2e}")
    assert np.array_equal(a, b), case


@pytest.mark.parametrize("planes", PLANES)
def test_stale_pad_rows_do_not_reach_the_result(rows, planes):
    """N = 257 leaves its V rows 67 .. 256 in the planes; the N = 67 evaluation after it reads rows 64 .. 127 in its last stage.
    The stale rows are finite (3 x the usual inputs): see the module docstring for what that does and does not show."""
    cfg = _cfg()
    saved = _lib.get_option("attn_f32_planes")
    eng = F5Engine(cfg, W.synth_state(W.f5_spec(cfg), 7), dtype="f32")
    try:
        _lib.set_option("attn_f32_planes", planes)
        assert _v_rows(eng) == 1
        x, c, d = _inputs(cfg, 257)
        eng.dit_eval(3.0 * x[None], 3.0 * c[None], 3.0 * d[None], K_EVAL)
        x, c, d = _inputs(cfg, 67)
        after = eng.dit_eval(x[None], c[None], d[None], K_EVAL)
    finally:
        _lib.set_option("attn_f32_planes", saved)
        eng.close()
    cfg = _cfg()
    eng = F5Engine(cfg, W.synth_state(W.f5_spec(cfg), 7), dtype="f32")
    try:
        _lib.set_option("attn_f32_planes", planes)
        fresh = eng.dit_eval(x[None], c[None], d[None], K_EVAL)
    finally:
        _lib.set_option("attn_f32_planes", saved)
        eng.close()
    assert np.isfinite(after).all() and np.array_equal(after, fresh)
    assert np.array_equal(fresh, rows[f"p{planes}.s2.n67"])


def test_v_rows_identical_run_to_run():
    cfg = _cfg()
    eng = F5Engine(cfg, W.synth_state(W.f5_spec(cfg), 7), dtype="f32")
    try:
        for N in (67, 700):
            x, c, d = _inputs(cfg, N)
            a = eng.dit_eval(x[None], c[None], d[None], K_EVAL)
            for _ in range(2):
                assert np.array_equal(a, eng.dit_eval(x[None], c[None], d[None], K_EVAL)), N
    finally:
        eng.close()
