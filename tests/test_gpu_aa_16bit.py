"""GPU: the anti-aliased SnakeBeta kernels in 16-bit storage — aa_act_pipe_kernel, its R = 8 and one-tile-per-workgroup variants,
the FAST math of aa_math.h and aa_conv_kernel<f16 | bf16> — elementwise against the float64 reference with the kernels' own
rounding points (tests/aa_ref64.py, where the bounds are derived).  Inputs are rounded to the storage type first, alpha and beta go
in with logscale=False, so the reference sees exactly what the kernels see.

Constants measured on the MI355X (256 CUs), and the gates that follow from them by rule:
  A_ACT     the absolute term of bound_act.  max(|y - ref| - 0.5 ulp16(ref) - P) over every case of (a), (b) and (d) up to 250
            revolutions: 1.24e-7 (f16, at 0.25 revolutions; bf16: never above 0).  The gate is twice that, rounded up to one digit:
            3e-7 (the rule's cap is 1e-4).  With the operation count of the up-sampler's chain in P (aa_ref64.phase_term(chain=...))
            the same maximum is below 0, so what is left is fp32 arithmetic, not v_sin_f32
  RMS_GATE  rms(y - R_q) / rms(q16(R_q) - R_q) of the fused kernel, largest over the cases of (e): f16 1.0027, bf16 1.0007.  The gate
            is 1.25 x that (the rule's cap is 1.5; the float32 oracle with the same rounding points sits at 1.001)
Beyond the documented +-256 revolutions of v_sin_f32 the kernels still follow the true sine (DESIGN.md, K-AA), so (d) runs to 1000.
"""
import functools

import numpy as np
import pytest

import aa_ref64 as R
from mi355tts import _lib
from mi355tts import bigvgan as BV
from mi355tts import weights as W

pytestmark = pytest.mark.gpu

DTYPES = ["f16", "bf16"]
LABEL = {"f16": "_Float16", "bf16": "__bf16"}
MEASURED_A_ACT = 1.24e-7
A_ACT = 3e-7
MEASURED_RMS = {"f16": 1.0027, "bf16": 1.0007}
RMS_GATE = {k: 1.25 * v for k, v in MEASURED_RMS.items()}


@pytest.fixture
def options():
    """set_option for a test; every key it set goes back to the value it had before."""
    saved = {}

    def set_option(key, value):
        saved.setdefault(key, _lib.get_option(key))
        _lib.set_option(key, value)
    yield set_option
    for k, v in saved.items():
        _lib.set_option(k, v)


@pytest.fixture(scope="module", autouse=True)
def _references_live_for_this_module_only():
    yield
    _act_case.cache_clear()


def _snake(C):
    """alpha, beta > 0 as float32, for logscale=False: what the library uploads is then exact."""
    return (np.exp(W.synth_normal(6, "a", (C,), std=0.3)).astype(np.float32),
            np.exp(W.synth_normal(7, "b", (C,), std=0.3)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _act_case(C, T, B, dtype, post, revs=None):
    """Inputs and reference of one activation case, computed once.  revs: alpha per channel such that the channel's largest
    |alpha U| / (2 pi) is that many revolutions."""
    x = R.q16(W.synth_normal(5, f"aa{C}{T}", (B, C, T), std=1.5), dtype)
    al, be = _snake(C)
    if revs is not None:
        _, p1 = R.activation1d_phase(x, np.ones(C, np.float32), be, post=post)
        al = (revs / p1.max(axis=(0, 2))).astype(np.float32)
    ref, phase, chain = R.activation1d_phase(x, al, be, post=post, chain=True)
    ib = R.snake_params(al, be)[1]
    return {"x": x.astype(np.float32), "al": al, "be": be, "ref": ref, "P": R.phase_term(phase, ib, post),
            "P_chain": R.phase_term(phase, ib, post, chain), "revs": float(phase.max())}


def _run_act(case, dtype, post):
    """(output as float64, labels of the aa_act launches)."""
    _lib.prof_reset(); _lib.prof_enable(("aa_act",))
    try:
        y = BV.aa_activation1d(case["x"], case["al"], case["be"], post=post, logscale=False, dtype=dtype)
        labels = {k["kernel"] for k in _lib.prof_kernels() if k["family"] == "aa_act" and k["launches"] > 0}
    finally:
        _lib.prof_enable(())
    return y.astype(np.float64), labels


def _check_act(tag, y, case, dtype):
    ref = case["ref"]
    assert y.shape == ref.shape
    over = np.abs(y - ref) - 0.5 * R.ulp16(ref, dtype)
    excess, excess_chain = float((over - case["P"]).max()), float((over - case["P_chain"]).max())
    print(f"AA16 {tag} {dtype} revs {case['revs']:.2f} excess {excess:.3e} (with the chain term {excess_chain:.3e}) gate {A_ACT:.1e}")
    bad = np.abs(y - ref) > R.bound_act(ref, case["P"], dtype, A_ACT)
    assert not bad.any(), (int(bad.sum()), excess, [tuple(int(i) for i in ix) for ix in np.argwhere(bad)[:5]])


# ---- (a) stand-alone activation, default path: pipelined, runs of 16 ------------------------------------------------------------------
ACT_SHAPES = [(8, 7, 3), (24, 1, 1), (24, 1000, 2), (48, 333, 1), (96, 41, 1),        # whole-C tiles: T < tile, T = 1, T % tile != 0
              (192, 70, 2), (1536, 9, 1),                                             # channel tiles of 64
              (104, 50, 1),                                                           # ... of 8
              (120, 50, 2)]                                                           # ... of 24


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("C,T,B", ACT_SHAPES)
def test_activation_default_path(C, T, B, post, dtype):
    case = _act_case(C, T, B, dtype, post)
    y, labels = _run_act(case, dtype, post)
    assert labels == {f"aa_act_pipe_kernel<{LABEL[dtype]}>"}
    _check_act(f"a C{C} T{T} B{B} post{int(post)}", y, case, dtype)


# ---- (b) workgroups that walk: tiles of 16 rows, three or four per workgroup ------------------------------------------------------------
def _channel_tile(C):
    """launch_t (csrc/aa_act.hip): all channels up to 96, else the largest of these that divides C."""
    return C if C <= 96 else next(c for c in (64, 48, 32, 24, 16, 8) if C % c == 0)


def _pipe_plan(C, T, B, post, tile_elems, run, cus):
    """The pipelined launch as launch_t decides it: (rows per tile, tiles, workgroups)."""
    CT = _channel_tile(C)
    TT = min(max(tile_elems // CT // run * run, run), 512)
    Tout = T + (30 if post else 0)
    ntiles = -(-Tout // TT) * (C // CT) * B
    xsp = -(-((TT + 10) * CT // 8) // 64) * 64 * 8
    lds = (2 * xsp + TT * CT) * 2
    return TT, ntiles, min(ntiles, cus * min(3, 160 * 1024 // lds))


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _walk_T(C, B):
    """T, not a multiple of 16, whose 16-row tiles number at least 3 * (3 * CUs) + 100 in the block form."""
    ntt = -(-(9 * _cus() + 100) // ((C // _channel_tile(C)) * B))
    return 16 * ntt - 7


WALK = [(24, 2), (192, 2)]                   # time tiles x items; time tiles x three channel tiles x items


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("C,B", WALK)
def test_activation_workgroups_walk_tiles(options, C, B, post, dtype):
    T, cus = _walk_T(C, B), _cus()
    tile = 16 * _channel_tile(C)
    TT, ntiles, grid = _pipe_plan(C, T, B, post, tile, 16, cus)
    assert TT == 16 and T % 16 != 0 and grid == 3 * cus and ntiles >= 3 * grid + 100      # every workgroup: three or four tiles
    case = _act_case(C, T, B, dtype, post)
    options("aa_tile", tile)
    y, labels = _run_act(case, dtype, post)
    assert labels == {f"aa_act_pipe_kernel<{LABEL[dtype]}>"}
    y2, _ = _run_act(case, dtype, post)
    assert np.array_equal(y, y2)
    _check_act(f"b C{C} T{T} B{B} post{int(post)} tiles {ntiles} workgroups {grid}", y, case, dtype)


# ---- (c) the variants compute the same thing, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("C,T,B", [(24, None, 2), (192, None, 2), (48, 333, 1), (192, 70, 2)])
def test_activation_variants_are_bit_identical(options, C, T, B, post, dtype):
    """aa_act.hip and aa_math.h claim bit-identical outputs for the streamed run of 16, the run of 8, the one-tile-per-workgroup
    kernel and every tile size."""
    T = T or _walk_T(C, B)
    case = _act_case(C, T, B, dtype, post)
    pipe, pipe8, plain = (f"aa_act_pipe_kernel<{LABEL[dtype]}>", f"aa_act_pipe_kernel<{LABEL[dtype]}>, runs of 8",
                          f"aa_act_kernel<{LABEL[dtype]}>")
    base, labels = _run_act(case, dtype, post)
    assert labels == {pipe}
    for tile in (16 * _channel_tile(C), 8192):
        options("aa_tile", tile)
        for (run, on, want) in [(16, 1, pipe), (8, 1, pipe8), (16, 0, plain), (8, 0, plain)]:
            options("aa_r", run); options("aa_pipe", on)
            y, labels = _run_act(case, dtype, post)
            assert labels == {want}, (tile, run, on)
            assert np.array_equal(y, base), (tile, run, on, int((y != base).sum()))


# ---- (d) phase range --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("revs", [0.25, 10.0, 100.0, 250.0, 600.0, 1000.0])
def test_activation_over_the_phase_range(revs, post, dtype):
    """v_sin_f32 takes revolutions, with nothing in front of it; P of the bound grows with the phase.  Its documented domain ends at
    256 revolutions: at 600 and 1000, 15 % and 38 % of the up-sampled samples lie beyond it, and a sine that returned 0 there would
    leave U in place of U + sin^2 / beta — an error of order 1 / beta."""
    case = _act_case(48, 500, 1, dtype, post, revs)
    assert abs(case["revs"] - revs) < 1e-3 * revs
    y, _ = _run_act(case, dtype, post)
    _check_act(f"d revs{revs:g} post{int(post)}", y, case, dtype)


# ---- (e) fused AA + conv ----------------------------------------------------------------------------------------------------------------------
FUSED = [(24, 3, 1, 700, 2), (24, 11, 5, 300, 1), (48, 7, 3, 515, 2), (96, 11, 5, 260, 1), (96, 3, 1, 130, 2), (16, 7, 1, 40, 1), (8, 3, 1, 5, 3),
         (40, 3, 1, 300, 1), (64, 7, 3, 300, 2), (72, 11, 5, 200, 1)]      # masked last 32 columns, both row strides, TN = 2 / 3 with C % 32 != 0


def _fused_inputs(C, k, T, B, dtype):
    x = R.q16(W.synth_normal(5, f"ac{C}{T}", (B, C, T), std=1.5), dtype)
    w = R.q16(W.synth_normal(8, f"w{C}{k}", (C, C, k), std=1.0 / np.sqrt(C * k)), dtype)
    bias = W.synth_normal(9, "bias", (C,), std=0.1)
    res = R.q16(W.synth_normal(10, f"r{C}{T}", (B, C, T)), dtype)
    return x, w, bias, res


def _run_fused(x, al, be, w, bias, d, res, dtype):
    _lib.prof_reset(); _lib.prof_enable(("conv_gemm",))
    try:
        y = BV.aa_conv1d(x, al, be, w, bias, dilation=d, res=res, logscale=False, dtype=dtype)
        labels = {k["kernel"] for k in _lib.prof_kernels() if k["family"] == "conv_gemm" and k["launches"] > 0}
    finally:
        _lib.prof_enable(())
    return y.astype(np.float64), labels


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("C,k,d,T,B", FUSED)
def test_fused_aa_conv(C, k, d, T, B, with_res, dtype):
    x, w, bias, res = _fused_inputs(C, k, T, B, dtype)
    res = res if with_res else None
    al, be = _snake(C)
    Rq, bound = R.fused(x, al, be, w, bias, d, res, dtype=dtype, A_act=A_ACT)
    y, labels = _run_fused(x, al, be, w, bias, d, res, dtype)
    assert labels == {f"aa_conv_kernel<{LABEL[dtype]}, {256 if C <= 48 else 128}, {(C + 31) // 32}>"}
    for _ in range(2):
        assert np.array_equal(_run_fused(x, al, be, w, bias, d, res, dtype)[0], y)
    err = np.abs(y - Rq)
    ratio = R.rms(y - Rq) / R.rms(R.q16(Rq, dtype) - Rq)
    print(f"AA16 e C{C} k{k} d{d} T{T} B{B} res{int(with_res)} {dtype} max err/bound {float((err / bound).max()):.3f} rms ratio {ratio:.4f}"
          f" gate {RMS_GATE[dtype]}")
    bad = err > bound
    assert not bad.any(), (int(bad.sum()), [tuple(int(i) for i in ix) for ix in np.argwhere(bad)[:5]])
    assert ratio <= RMS_GATE[dtype], ratio


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [2100, None])
def test_fused_one_and_two_workgroups_per_cu_are_bit_identical(options, T, dtype):
    """aaconv_lds_min = 83968 leaves room for one workgroup per CU; the default is two, the mode in which rounds 1-2 were not
    reproducible.  (96, 11, 5, 2100, 8) is 17 x 8 tiles of 128 rows, which the dispatcher may or may not pair on a CU; the second
    T gives more tiles than the device has CUs, so some are paired whatever it does."""
    C, k, d, B = 96, 11, 5, 8
    T = T or 128 * (_cus() // B + 1) - 28
    x, w, bias, res = _fused_inputs(C, k, T, B, dtype)
    al, be = _snake(C)
    y2 = _run_fused(x, al, be, w, bias, d, res, dtype)[0]
    assert np.array_equal(_run_fused(x, al, be, w, bias, d, res, dtype)[0], y2)
    options("aaconv_lds_min", 83968)
    y1 = _run_fused(x, al, be, w, bias, d, res, dtype)[0]
    assert np.array_equal(y1, y2), int((y1 != y2).sum())
