"""GPU: the store policy of the exact-fit fp32 linears' epilogues (MI355TTS_EPI_WT, csrc/options.h; store16, csrc/lds_dma.h)
changes no result.  Write-through stores carry the same values to the same addresses as plain ones, and the whole-line form of
the O / FF2 rows only changes which lane stores which 16 bytes, so a DiT evaluation is equal in EVERY element whatever the mask.

The model is the full-width one of tests/test_gpu_attention_dispatch.py ("mid": dim 1024, 16 heads, one block).  Cases:
  * N = 449, one utterance (898 rows), and the ragged pair (225, 67): the smallest shapes at which the AdaLN-fold / panel-plane
    forms run.  898 rows are six row groups of 144 and one of 34 rows: the masked last row group is covered.  gemm_x3d_min_eff is
    lowered so that all four linears of the block and the input projection take linear_x3d_kernel (QKV at tile width 128, FF1 and
    O / FF2 at 64, i.e. the half-block form of the residual epilogue); the profiler labels must show each role.
  * N = 1126, one utterance, at the default threshold: the 16 x 16-tile shape of the benchmark (QKV at 192, FF1 at 128, O / FF2 at 64).
The mask is read once per process, so mask 0 and mask 31 run in child processes (this file is the child's script), the default
mask in this one.  Under mask 31 every case is evaluated twice: run to run equal."""
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

K_EVAL = 1
N_ONE = 449
RAGGED = (225, 67)
N_FULL = 1126
ROLES = ("AdaLN fold, QKV", "AdaLN fold, FF1", "AdaLN fold, O / FF2", "rows out")
SMALL = ("n449", "ragged.u0", "ragged.u1")


def _mid_cfg():
    """tests/test_gpu_attention_dispatch.py, model "mid": full-width layers, one block"""
    return F5Config(depth=1, text_dim=64, text_num_embeds=40, conv_layers=1, vocos_dim=64, vocos_intermediate=128, vocos_layers=1,
                    nfe_step=4)


def _inputs(cfg, N, seed=0):
    cd = cfg.mel_dim + cfg.text_dim
    return (W.synth_normal(3 + seed, f"n{N}", (N, cfg.mel_dim)), W.synth_normal(4 + seed, f"c{N}", (N, cd), std=0.7),
            W.synth_normal(5 + seed, f"d{N}", (N, cd), std=0.7))


def _profiled(call):
    _lib.prof_reset(); _lib.prof_enable(("conv_gemm",))
    try:
        a = call()
    finally:
        _lib.prof_enable(())
    return a, {k["kernel"]: k["launches"] for k in _lib.prof_kernels() if k["launches"] > 0}


def _roles_launched(kernels):
    """1 per role of ROLES when some linear_x3d_kernel launch carried its label"""
    return np.asarray([int(any(k.startswith("linear_x3d_kernel<") and k.endswith(", " + r + ">") for k in kernels)) for r in ROLES])


def _evaluate(full, twice):
    """name -> evaluation (and name + ".again" with `twice`), "roles.*" -> which x3d roles launched, "saturation_events"."""
    cfg = _mid_cfg()
    eng = F5Engine(cfg, W.synth_state(W.f5_spec(cfg), 7), dtype="f32")
    out = {}
    saved = _lib.get_option("gemm_x3d_min_eff")
    try:
        x, c, d = _inputs(cfg, N_ONE)
        ins = [_inputs(cfg, n, seed=10 * u) for u, n in enumerate(RAGGED)]
        one = lambda: eng.dit_eval(x[None], c[None], d[None], K_EVAL)
        rag = lambda: eng.dit_eval_ragged([i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins], K_EVAL)
        _lib.set_option("gemm_x3d_min_eff", 1)
        try:
            out["n449"], k = _profiled(one)
            out["roles.n449"] = _roles_launched(k)
            r, k = _profiled(rag)
            out["roles.ragged"] = _roles_launched(k)
            for u in range(len(RAGGED)):
                out[f"ragged.u{u}"] = r[u]
            if twice:
                out["n449.again"] = one()
                for u, a in enumerate(rag()):
                    out[f"ragged.u{u}.again"] = a
        finally:
            _lib.set_option("gemm_x3d_min_eff", saved)
        if full:
            x, c, d = _inputs(cfg, N_FULL)
            out["full"], k = _profiled(lambda: eng.dit_eval(x[None], c[None], d[None], K_EVAL))
            out["roles.full"] = _roles_launched(k)
        out["saturation_events"] = np.asarray(eng.info()["saturation_events"])
    finally:
        eng.close()
    return out


if __name__ == "__main__":
    np.savez(sys.argv[1], **_evaluate(full=True, twice=True))
    sys.exit(0)


def _child(mask):
    env = dict(os.environ, MI355TTS_EPI_WT=str(mask))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "out.npz")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        with np.load(path) as z:
            return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def default_mask():
    return _evaluate(full=False, twice=False)


@pytest.fixture(scope="module")
def mask0():
    return _child(0)


@pytest.fixture(scope="module")
def mask31():
    return _child(31)


def test_every_role_launched_on_the_exact_fit_kernel(default_mask, mask0, mask31):
    for name, got in (("default", default_mask), ("0", mask0), ("31", mask31)):
        for key in ("roles.n449", "roles.ragged") + (("roles.full",) if name != "default" else ()):
            missing = [r for r, n in zip(ROLES, got[key]) if not n]
            assert not missing, f"mask {name}, {key}: no linear_x3d_kernel launch for {missing}"


@pytest.mark.parametrize("case", SMALL)
def test_results_equal_under_every_mask(default_mask, mask0, mask31, case):
    d, a, b = default_mask[case], mask0[case], mask31[case]
    assert d.shape == a.shape == b.shape and np.isfinite(a).all()
    print(f"{case}: elements that differ, mask 0 vs 31: {int((a != b).sum())}; default vs 0: {int((d != a).sum())}")
    assert np.array_equal(a, b), case
    assert np.array_equal(d, a), case
    assert np.array_equal(d, b), case


def test_range_watch_equal_under_every_mask(default_mask, mask0, mask31):
    s = [int(g["saturation_events"]) for g in (default_mask, mask0, mask31)]
    assert s[0] == s[1] == s[2], s


@pytest.mark.parametrize("case", SMALL)
def test_run_to_run_equal_with_write_through_stores(mask31, case):
    assert np.array_equal(mask31[case], mask31[case + ".again"]), case


def test_benchmark_shape_equal_with_plain_and_write_through_stores(mask0, mask31):
    a, b = mask0["full"], mask31["full"]
    assert a.shape == b.shape == (2, N_FULL, _mid_cfg().mel_dim) and np.isfinite(a).all()
    print(f"N = {N_FULL}: elements that differ, mask 0 vs 31: {int((a != b).sum())}")
    assert np.array_equal(a, b)
