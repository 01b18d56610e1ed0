"""GPU: the decode-step linear kernels of the IndexTTS GPT (csrc/gpt.hip gemv_d_kernel, gemv_b_kernel, gemm_skinny_kernel,
gemm_skinny_wide_kernel), one launch at a time through the unit entries mi_gpt_linear_decode / mi_gpt_linear_batch (the engine's
own launchers launch_gpt_gemv / launch_gpt_gemv_b), against the float64 reference tests/gpt_linear_ref.py.  The library profiler's
kernel label of every launch says which instantiation ran; the last test asserts that the file reached every instantiation the
dispatch can reach on this device (the dispatch rules are restated below, from the device's CU count).

Exact family (the forms without LayerNorm): small-integer inputs, every sum exact in fp32 in any order — the result must be
np.array_equal to the integer reference (fp32 output) or to its rounding (16-bit output).  No tolerance.

Random family: w std 0.05, x std 1, LayerNorm gains near 1, evaluated on inputs already rounded to the type under test.  Per
element |out - ref| <= G * 2^-24 * sum_k |w x'|  (+ A_GELU * max(1, |v|) with the activation, v the value before it)
(+ one unit in the last place of a 16-bit output, ulp_bar).  G per kernel family and A_GELU are MEASURED here, against the
reference alone, as the worst |out - ref| / (2^-24 sum |w x'|) over this file's fp32-output cases without activation, and the
worst |out - ref| / max(1, |v|) over its fp32-output cases with it; the gate is twice the measured value rounded up to one
digit.  Caps that the gates must respect whatever was measured (asserted per case): G <= K / 64 + 12 on the VALU kernels (serial
depth per lane, the wave tree, the LayerNorm roundings), G <= K / (8 KS) + 12 on the matrix-core kernels, A_GELU <= 2e-5.
pre_out against the float64 LayerNorm at 2e-5 * max |row|.

Measured on an MI355X (256 CUs; printed at the end of a run with -s), and the gates that follow:

    family                                   measured G   gate    set by
    gemv_d plain, fp32        d_plain_f32      1.903        4     K = 2856, N = 37, with res
    gemv_d plain, 16-bit      d_plain_16       3.129        7     bf16, K = 5120
    gemv_d LayerNorm, fp32    d_ln_f32         2.047        5     K = 40, N = 6152 (R = 4)
    gemv_d LayerNorm, 16-bit  d_ln_16          2.939        6     bf16, K = 2600, N = 8200 (R = 5)
    gemv_d LN + leading LN    d_pre_f32        0.579        2     K = 320
    the same, 16-bit          d_pre_16         2.232        5     bf16, K = 320
    gemv_b (all three types)  gemv_b           3.070        7     f16, K = 8, N = 4101, 8 rows
    gemm_skinny(_wide)        mfma             1.365        3     f16, K = 256, N = 4101, 48 rows
    A_GELU                                     1.532e-6     4e-6

Every gate is below the smallest cap of its family (12.125 at K = 8).  Wall time of the file: 13 s for its 181 tests, the
slowest (the LayerNorm form's KI = 8 sweep over R at 16 bits, N up to 8200 x K = 3624) 0.35 s.

The random family's bias and residual are drawn at the scale of the sums (std 0.025 sqrt(K) and 0.05 sqrt(K)): the bar counts the
products alone, and a first measurement with bias std 0.1 and res std 1 read G = 10.4 at K = 8, N = 37 — the rounding of the final
`+ res`, which is half a unit in the last place of |res| whatever the kernel does.  At K = 8 the random family runs without them;
the exact family carries bias and residual at every K.

A ragged K here ends 40 elements into the last 64-lane iteration: on an 8-element boundary, five 16-byte lanes (16-bit) or ten
(fp32) into it, and no multiple of 16 elements.
"""
import functools

import numpy as np
import pytest

import gpt_linear_ref as R
from mi355tts import _lib
from mi355tts.indextts import linear_batch, linear_batch_rows, linear_decode

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "f16", "bf16"]
BITS16 = ["f16", "bf16"]
TL = {"f32": "float", "f16": "_Float16", "bf16": "__bf16"}
NAN = np.float32(np.nan)
# gate = 2 x measured, one digit up (module docstring); family -> G
GATE = {"d_plain_f32": 4.0, "d_plain_16": 7.0, "d_ln_f32": 5.0, "d_ln_16": 6.0, "d_pre_f32": 2.0, "d_pre_16": 5.0,
        "gemv_b": 7.0, "mfma": 3.0}
A_GELU = 4e-6
MEASURED_G, MEASURED_A, SEEN = {}, [0.0], set()
KI_PLAIN = [1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 32]
KI_LN = [1, 2, 3, 4, 5, 6, 8]


# ---------------------------------------------------------------------------------------------------------------
# the dispatch rules of csrc/gpt.hip, restated
# ---------------------------------------------------------------------------------------------------------------
def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _v(dtype):
    return 4 if dtype == "f32" else 8


def _ki(k, dtype, ln):
    ki = -(-k // (64 * _v(dtype)))
    return next(t for t in (KI_LN if ln else KI_PLAIN) if t >= ki)


def _r_ln(n, qkv):
    r = 1
    while r < (2 if qkv else 5) and -(-n // (8 * r)) > _cus():
        r += 1
    return r


def _b(v):
    return "true" if v else "false"


def d_label(dtype, k, n, ln=False, qkv=False):
    r = _r_ln(n, qkv) if ln else 1
    return f"gemv_d_kernel<{TL[dtype]}, {r}, {_ki(k, dtype, ln)}, {8 if ln else 4}, {_b(ln)}, {_b(qkv)}>"


def b_label(dtype, nb, n, qkv=False):
    bb = 2 if nb <= 2 else 4 if nb <= 4 else 8 if nb <= 8 else 16
    return f"gemv_b_kernel<{TL[dtype]}, {2 if n >= 4096 else 1}, {bb}, {_b(qkv)}>"


def _ks(k):
    return 8 if k > 2048 else 4


def _unr(k):
    return 5 if (k // _ks(k)) % 320 == 0 else 1


def s_label(dtype, k, qkv=False):
    return f"gemm_skinny_kernel<{TL[dtype]}, {_b(qkv)}, {_unr(k)}>"


def w_label(dtype, k, nb, qkv=False):
    return f"gemm_skinny_wide_kernel<{TL[dtype]}, {_b(qkv)}, {_unr(k)}, {-(-nb // 16)}>"


def _qkv_r_reachable(dtype, ki):
    """R of the QKV form at this KI: n = 3 k, k a multiple of 64 inside the KI's range and the LayerNorm's limit"""
    return sorted({_r_ln(3 * k, True) for k in range(64, 64 * _v(dtype) * 8 + 1, 64) if _ki(k, dtype, True) == ki})


def _qkv_k(dtype, ki, r):
    return next(k for k in range(64, 64 * _v(dtype) * 8 + 1, 64) if _ki(k, dtype, True) == ki and _r_ln(3 * k, True) == r)


def reachable():
    s = set()
    for dt in DTYPES:
        s |= {f"gemv_d_kernel<{TL[dt]}, 1, {ki}, 4, false, false>" for ki in KI_PLAIN}
        for ki in KI_LN:
            s |= {f"gemv_d_kernel<{TL[dt]}, {r}, {ki}, 8, true, false>" for r in range(1, 6)}
            s |= {f"gemv_d_kernel<{TL[dt]}, {r}, {ki}, 8, true, true>" for r in _qkv_r_reachable(dt, ki)}
        s |= {f"gemv_b_kernel<{TL[dt]}, {r}, {bb}, {q}>" for r in (1, 2) for bb in (2, 4, 8, 16) for q in ("true", "false")}
    for dt in BITS16:
        s |= {f"gemm_skinny_kernel<{TL[dt]}, {q}, {u}>" for q in ("true", "false") for u in (1, 5)}
        s |= {f"gemm_skinny_wide_kernel<{TL[dt]}, {q}, {u}, {ct}>" for q in ("true", "false") for u in (1, 5) for ct in (2, 3, 4)}
    return s


# ---------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def _profiled():
    keep = _lib.get_option("gpt_mfma_min")
    _lib.prof_enable(("conv_gemm",))
    try:
        yield
    finally:
        _lib.prof_enable(())
        _lib.set_option("gpt_mfma_min", keep)
        print("\ngpt linear, measured G (worst |out - ref| / (2^-24 sum |w x'|), fp32 output, no activation): "
              + ", ".join(f"{f} {MEASURED_G.get(f, 0.0):.3f}" for f in GATE) + f"; A_GELU {MEASURED_A[0]:.3e}")


@pytest.fixture
def mfma_min():
    """set the option "gpt_mfma_min" for one test"""
    keep = _lib.get_option("gpt_mfma_min")
    yield lambda v: _lib.set_option("gpt_mfma_min", v)
    _lib.set_option("gpt_mfma_min", keep)


def _launch(fn, label):
    """one launch under the profiler: its conv_gemm family label must be `label`"""
    _lib.prof_reset()
    r = fn()
    seen = {k["kernel"] for k in _lib.prof_kernels() if k["family"] == "conv_gemm" and k["launches"] > 0}
    SEEN.update(seen)
    assert seen == ({label} if isinstance(label, str) else set(label)), (seen, label)
    return r


def _rng(*key):
    return np.random.default_rng([9527, *key])


@functools.lru_cache(maxsize=2)
def _weights(n, k, dtype):
    """(n, k) weights, std 0.05, rounded to dtype, as float32 and float64; a large matrix is a pool of 2^20 + 7 values laid out
    cyclically (the odd length keeps rows apart)"""
    pool = R.round_to(_rng(n, k).normal(0, 0.05, min(n * k, (1 << 20) + 7)), dtype)
    w = np.resize(pool, (n, k))
    return w, w.astype(np.float64)


def _bias_res(r, k, bshape, rshape, res):
    """bias and residual of the random family at the scale of the sums, 0.05 sqrt(k) (bias half of it): the bar counts the products
    alone, so operands that dwarf them would measure the final additions, not the kernel.  At k = 8 a sum can be almost nothing:
    there the random family runs without them, and the exact family carries the bias and the residual."""
    if k <= 8:
        return None, None
    sc = 0.05 * np.sqrt(k)
    return r.normal(0, 0.5 * sc, bshape).astype(np.float32), (r.normal(0, sc, rshape).astype(np.float32) if res else None)


def _ln_vec(k, *key):
    r = _rng(k, *key)
    return (1 + r.normal(0, 0.1, k)).astype(np.float32), r.normal(0, 0.1, k).astype(np.float32)


def _cap(fam, k):
    return k / (8 * _ks(k)) + 12 if fam == "mfma" else k / 64 + 12


def _check(out, ref, fam, dtype, k, out_f32, act, what):
    """out against R.linear()'s dict, every element; feeds the measurements"""
    assert GATE[fam] <= _cap(fam, k) and A_GELU <= 2e-5, "a gate exceeds its cap"
    want, base = ref["out"], 2.0 ** -24 * ref["mag"]
    assert out.shape == want.shape and np.isfinite(out).all(), (what, "non-finite output")
    err = np.abs(out.astype(np.float64) - want)
    amp = np.maximum(1.0, np.abs(ref["v"]))
    if out_f32 and not act:
        MEASURED_G[fam] = max(MEASURED_G.get(fam, 0.0), float((err / np.maximum(base, 1e-300)).max()))
    if out_f32 and act:
        MEASURED_A[0] = max(MEASURED_A[0], float((err / amp).max()))
    bar = GATE[fam] * base + (A_GELU * amp if act else 0.0) + (0.0 if out_f32 else R.ulp_bar(want, dtype))
    ratio = err / np.maximum(bar, 1e-300)
    worst = float(ratio.max())
    print(f"{what} [{dtype}] {fam}: worst err / bar {worst:.3f}, err / (2^-24 mag) {float((err / np.maximum(base, 1e-300)).max()):.3f}")
    assert worst <= 1.0, (what, dtype, fam, worst, np.unravel_index(int(ratio.argmax()), ratio.shape))


def _fam_d(dtype, ln, pre):
    return ("d_pre_" if pre else "d_ln_" if ln else "d_plain_") + ("f32" if dtype == "f32" else "16")


def _sentinel(shape):
    """cache filler, exact in bf16, no two neighbours alike"""
    i = np.arange(int(np.prod(shape)), dtype=np.int64)
    return (64.0 + ((i * 7) % 31) * 0.5).astype(np.float32).reshape(shape)          # 64 .. 79: eight significant bits


def _decode_case(dtype, n, k, *, ln=False, pre=False, act=False, res=False, out_f32=True, hist=None, S=6, key=0):
    """one random-family launch of the single-row kernel, checked; hist != None: the QKV form"""
    w, w64 = _weights(n, k, dtype)
    r = _rng(n, k, key)
    x = r.normal(0, 1, k).astype(np.float32)
    if pre:
        x = (2 * x + 0.5).astype(np.float32)
    if not ln:
        x = R.round_to(x, dtype)
    bias, rs = _bias_res(r, k, (n,), (n,), res)
    lnv = _ln_vec(k, 1) if ln else None
    prev = _ln_vec(k, 2) if pre else None
    cache = (_sentinel((k // 64, S, 64)), _sentinel((k // 64, S, 64)) + 1) if hist is not None else None
    what = f"decode n={n} k={k} ln={ln} pre={pre} act={act} res={res} of={out_f32} hist={hist}"
    got = _launch(lambda: linear_decode(w, x, bias=bias, ln=lnv, pre=prev, res=rs, act=act, out_f32=out_f32, cache=cache,
                                        hist=hist or 0, dtype=dtype), d_label(dtype, k, n, ln, hist is not None))
    ref = R.linear(w64, x, bias, rs, act, lnv, prev)
    fam = _fam_d(dtype, ln, pre)
    if pre:
        e = np.abs(got["pre_out"].astype(np.float64) - ref["pre_out"]).max()
        assert np.isfinite(got["pre_out"]).all() and e <= 2e-5 * np.abs(ref["pre_out"]).max(), (what, e)
    if hist is None:
        _check(got["out"], ref, fam, dtype, k, out_f32, act, what)
        return
    # QKV: the q third in `out`, the rest of `out` untouched (NaN); row hist of the caches, nothing else
    q = {kk: ref[kk][:k] for kk in ("out", "mag", "v")}
    _check(got["out"][:k], q, fam, dtype, k, out_f32, act, what + " q")
    assert np.isnan(got["out"][k:]).all(), (what, "the k / v thirds of out were written")
    for name, c0, lo in (("K", cache[0], k), ("V", cache[1], 2 * k)):
        c1 = got[name]
        rest = np.ones(c0.shape, bool)
        if hist < S:
            rest[:, hist] = False
            part = {kk: ref[kk][lo:lo + k].reshape(k // 64, 64) for kk in ("out", "mag", "v")}
            _check(c1[:, hist], part, fam, dtype, k, False, act, what + " " + name)
            assert (c1[:, hist] != c0[:, hist]).all(), (what, name, "row hist still holds the sentinel")
        assert np.array_equal(c1[rest], c0[rest]), (what, name, "a cache element outside row hist changed")


def _exact_decode(dtype, n, k, res, out_f32):
    w, x, bias, rs = R.exact_case(n, k, 1, with_res=res)
    got = _launch(lambda: linear_decode(w, x[0], bias=bias, res=rs[0] if res else None, out_f32=out_f32, dtype=dtype),
                  d_label(dtype, k, n))["out"]
    want = R.linear(w, x[0], bias, rs[0] if res else None)["out"]
    want = want.astype(np.float32) if out_f32 else R.round_to(want, dtype)
    assert np.array_equal(got, want), (dtype, n, k, res, out_f32, np.flatnonzero(got != want)[:8])


# ---------------------------------------------------------------------------------------------------------------
# gemv_d_kernel
# ---------------------------------------------------------------------------------------------------------------
def _two_k(dtype, ki):
    per = 64 * _v(dtype)
    return [ki * per, (ki - 1) * per + 40]


@pytest.mark.parametrize("ki", KI_PLAIN)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemv_d_plain_every_ki(dtype, ki):
    """N = 37 (rows end inside a block), the full and a ragged K of every KI, with and without res, fp32 and T output"""
    for k in _two_k(dtype, ki):
        assert _ki(k, dtype, False) == ki
        for res in (False, True):
            for of in (True, False):
                if k <= R.K_EXACT_MAX:
                    _exact_decode(dtype, 37, k, res, of)
                _decode_case(dtype, 37, k, res=res, out_f32=of)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemv_d_plain_k8(dtype):
    for of in (True, False):
        for res in (False, True):
            _exact_decode(dtype, 37, 8, res, of)
        _decode_case(dtype, 37, 8, out_f32=of)


@pytest.mark.parametrize("ki", KI_LN)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemv_d_ln_every_ki_and_r(dtype, ki):
    """fused LayerNorm: R = 1 at N = 37 with the full and a ragged K, with the activation and both output types; then every
    R in 2 .. 5 at its smallest N, and the QKV form at every R it can have at this KI"""
    for k in _two_k(dtype, ki):
        assert _ki(k, dtype, True) == ki
        for act, of in ((False, True), (True, True), (True, False), (False, False)):
            _decode_case(dtype, 37, k, ln=True, act=act, out_f32=of)
    k = _two_k(dtype, ki)[1]
    for r in range(2, 6):
        n = 8 * _cus() * (r - 1) + 8
        assert _r_ln(n, False) == r
        _decode_case(dtype, n, k, ln=True)
    for r in _qkv_r_reachable(dtype, ki):
        kq = _qkv_k(dtype, ki, r)
        _decode_case(dtype, 3 * kq, kq, ln=True, out_f32=False, hist=2)


@pytest.mark.parametrize("r", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemv_d_ln_both_sides_of_every_r_boundary(dtype, r):
    """KI = 1 (K = 256): the smallest and the largest N that run R rows per wave on this device"""
    for n in (8 * _cus() * (r - 1) + 8, 8 * _cus() * r):
        assert _r_ln(n, False) == r
        _decode_case(dtype, n, 256, ln=True, act=r % 2 == 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemv_d_indextts_1_5_shapes(dtype):
    """hidden 1280: the QKV layer, the MLP's first layer with gelu_new, the head behind ln_f and final_norm"""
    _decode_case(dtype, 3840, 1280, ln=True, out_f32=False, hist=3)
    _decode_case(dtype, 5120, 1280, ln=True, act=True, out_f32=False)
    _decode_case(dtype, 5120, 1280, ln=True, act=True)
    _decode_case(dtype, 8194, 1280, ln=True, pre=True)


@pytest.mark.parametrize("k", [320, 1280, 2048])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemv_d_leading_layernorm(dtype, k):
    _decode_case(dtype, 37, k, ln=True, pre=True)
    _decode_case(dtype, 37, k, ln=True, pre=True, act=True, out_f32=False)


@pytest.mark.parametrize("hist", [0, 1, 5, 6])
@pytest.mark.parametrize("k", [128, 704])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemv_d_qkv_cache_row(dtype, k, hist):
    """R = 1 (k = 128) and R = 2 (k = 704, 11 heads), max_seq = 6: hist 0, 1, max_seq - 1 and max_seq (nothing is written)"""
    assert _r_ln(3 * k, True) == (1 if k == 128 else 2)
    _decode_case(dtype, 3 * k, k, ln=True, out_f32=False, hist=hist, S=6)
    _decode_case(dtype, 3 * k, k, ln=True, out_f32=True, hist=hist, S=6, key=1)


def _refused(fn, text):
    with pytest.raises(_lib.MiError, match=text):
        fn()


@pytest.mark.parametrize("dtype", DTYPES)
def test_bad_arguments_are_refused_and_the_next_call_works(dtype):
    lim = 2048 if dtype == "f32" else 4096
    z = lambda *s: np.zeros(s, np.float32)
    ln = lambda k: (z(k) + 1, z(k))
    cache = lambda k: (z(k // 64, 4, 64), z(k // 64, 4, 64))
    _refused(lambda: linear_decode(z(8, lim + 8), z(lim + 8), ln=ln(lim + 8), dtype=dtype), "fused LayerNorm supports K <= %d" % lim)
    _refused(lambda: linear_decode(z(8, 2056), z(2056), ln=ln(2056), pre=ln(2056), dtype=dtype), "LayerNorm supports K <= 2048")
    _refused(lambda: linear_decode(z(8, 12), z(12), dtype=dtype), "multiple of 8")
    _refused(lambda: linear_batch(z(8, 12), z(2, 12), dtype=dtype), "multiple of 8")
    _refused(lambda: linear_decode(z(8, 64), z(64), ln=ln(64), res=z(8), dtype=dtype), "no residual")
    _refused(lambda: linear_decode(z(192, 64), z(64), cache=cache(64), dtype=dtype), "QKV epilogue comes with the fused LayerNorm")
    _refused(lambda: linear_decode(z(193, 64), z(64), ln=ln(64), cache=cache(64), dtype=dtype), "multiple of 3")
    _refused(lambda: linear_batch(z(193, 64), z(2, 64), cache=(z(2, 1, 4, 64), z(2, 1, 4, 64)), hist=[0, 0], dtype=dtype), "multiple of 3")
    _refused(lambda: linear_decode(z(8, 64), z(64), pre=ln(64), dtype=dtype), "leading LayerNorm comes with the fused one")
    with pytest.raises((ValueError, _lib.MiError)):
        linear_batch(z(8, 64), z(65, 64), dtype=dtype)
    assert _lib.load().mi_gpt_linear_batch_rows(65) < 0 and _lib.load().mi_gpt_linear_batch_rows(0) < 0
    assert [linear_batch_rows(n) for n in (1, 2, 3, 5, 9, 17, 64)] == [2, 2, 4, 8, 16, 32, 64]
    _exact_decode(dtype, 37, 72, True, True)
    if dtype != "f32":
        _decode_case(dtype, 37, 4096, ln=True)          # the widest row the 16-bit LayerNorm form holds


# ---------------------------------------------------------------------------------------------------------------
# gemv_b_kernel
# ---------------------------------------------------------------------------------------------------------------
def _batch_label(dtype, nb, n, k, qkv=False):
    """what launch_gpt_gemv_b runs at the options in force"""
    mfma = dtype != "f32" and nb >= _lib.get_option("gpt_mfma_min") and k % (_ks(k) * 64) == 0
    if mfma:
        return s_label(dtype, k, qkv) if nb <= 16 else w_label(dtype, k, nb, qkv)
    return {b_label(dtype, min(16, nb - b0), n, qkv) for b0 in range(0, nb, 16)}


def _batch_fam(label):
    return "mfma" if isinstance(label, str) and label.startswith("gemm_skinny") else "gemv_b"


def _batch_random(dtype, nb, n, k, *, act=False, res=False, out_f32=True, hist=None, S=6, key=0):
    w, w64 = _weights(n, k, dtype)
    r = _rng(n, k, nb, key)
    x = R.round_to(r.normal(0, 1, (nb, k)), dtype)
    bias, rs = _bias_res(r, k, (n,), (nb, n), res)
    qkv = hist is not None
    cache = (_sentinel((nb, k // 64, S, 64)), _sentinel((nb, k // 64, S, 64)) + 1) if qkv else None
    label = _batch_label(dtype, nb, n, k, qkv)
    fam = _batch_fam(label)
    what = f"batch nb={nb} n={n} k={k} act={act} res={res} of={out_f32} hist={hist}"
    got = _launch(lambda: linear_batch(w, x, bias=bias, res=rs, act=act, out_f32=out_f32, cache=cache, hist=hist,
                                       x_dead=np.full(k, NAN), dtype=dtype), label)
    ref = R.linear(w64, x, bias, rs, act)
    assert np.isnan(got["out"][nb:]).all(), (what, "a row at or beyond nb was written")
    if not qkv:
        _check(got["out"][:nb], ref, fam, dtype, k, out_f32, act, what)
        return got
    _check(got["out"][:nb, :k], {kk: ref[kk][:, :k] for kk in ("out", "mag", "v")}, fam, dtype, k, out_f32, act, what + " q")
    assert np.isnan(got["out"][:nb, k:]).all(), (what, "the k / v thirds of out were written")
    for name, c0, lo in (("K", cache[0], k), ("V", cache[1], 2 * k)):
        c1 = got[name]
        rest = np.ones(c0.shape, bool)
        for b in range(nb):
            if hist[b] < S:
                rest[b, :, hist[b]] = False
                part = {kk: ref[kk][b, lo:lo + k].reshape(k // 64, 64) for kk in ("out", "mag", "v")}
                _check(c1[b, :, hist[b]], part, fam, dtype, k, False, act, what + f" {name} slot {b}")
                assert (c1[b, :, hist[b]] != c0[b, :, hist[b]]).all()
        assert np.array_equal(c1[rest], c0[rest]), (what, name, "a cache element outside the slots' rows changed")
    return got


def _batch_exact(dtype, nb, n, k, res, out_f32):
    w, x, bias, rs = R.exact_case(n, k, nb, with_res=res)
    got = _launch(lambda: linear_batch(w, x, bias=bias, res=rs, out_f32=out_f32, x_dead=np.full(k, NAN), dtype=dtype),
                  _batch_label(dtype, nb, n, k))["out"]
    want = R.linear(w, x, bias, rs)["out"]
    want = want.astype(np.float32) if out_f32 else R.round_to(want, dtype)
    assert np.array_equal(got[:nb], want), (dtype, nb, n, k, res, out_f32, np.argwhere(got[:nb] != want)[:8])
    assert np.isnan(got[nb:]).all()
    return got


NB_B = [1, 2, 3, 4, 5, 8, 9, 16]
K_B = [8, 1016, 1024, 1032, 2056, 5120]


@pytest.mark.parametrize("nb", NB_B)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemv_b_every_width_and_chunk_tail(dtype, nb, mfma_min):
    """N = 37 (R = 1) at every K: below a chunk, a chunk's tail, the exact chunk, just past it, two chunks and a tail, five
    chunks; N = 4101 (R = 2) at K = 8 and 1032.  x rows at and beyond nb are NaN."""
    mfma_min(65)
    for n, ks in ((37, K_B), (4101, [8, 1032])):
        for i, k in enumerate(ks):
            _batch_exact(dtype, nb, n, k, res=i % 2 == 0, out_f32=i % 3 != 0)
            _batch_random(dtype, nb, n, k, res=i % 2 == 1, out_f32=True)
            _batch_random(dtype, nb, n, k, act=True, out_f32=i % 2 == 0)


@pytest.mark.parametrize("nb", [2, 3, 5, 9])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemv_b_qkv_per_slot_rows(dtype, nb, mfma_min):
    """R = 1 (k = 128) and R = 2 (k = 1408, n = 4224): every slot its own hist, one of them max_seq"""
    mfma_min(65)
    hist = [(3 * b + 1) % 6 for b in range(nb)]
    hist[nb // 2] = 6
    for k in (128, 1408):
        _batch_random(dtype, nb, 3 * k, k, out_f32=False, hist=hist, S=6)


@pytest.mark.parametrize("nb", [17, 40])
def test_gemv_b_fp32_groups_of_16(nb):
    """fp32 above 16 rows walks groups of 16: every row equals, bit for bit, the row computed alone"""
    n, k = 37, 1032
    got = _batch_random("f32", nb, n, k, res=True)["out"]
    _batch_exact("f32", nb, n, k, True, True)
    w, _ = _weights(n, k, "f32")
    r = _rng(n, k, nb, 0)
    x = R.round_to(r.normal(0, 1, (nb, k)), "f32")
    bias, rs = _bias_res(r, k, (n,), (nb, n), True)
    for b in range(nb):
        alone = _launch(lambda: linear_batch(w, x[b:b + 1], bias=bias, res=rs[b:b + 1], dtype="f32"), b_label("f32", 1, n))["out"]
        assert np.array_equal(alone[0], got[b]), (nb, b)


# ---------------------------------------------------------------------------------------------------------------
# the matrix-core kernels (16-bit types)
# ---------------------------------------------------------------------------------------------------------------
K_S = [256, 1024, 1280, 2048, 2560, 4096, 5120]


@pytest.mark.parametrize("k", K_S)
@pytest.mark.parametrize("dtype", BITS16)
def test_gemm_skinny(dtype, k, mfma_min):
    """KS = 4 up to K = 2048, 8 above; UNR = 5 at K = 1280, 2560, 5120; N = 16 (one tile) and 301 (ragged last tile)"""
    for nb in (9, 13, 16, 3):
        mfma_min(2 if nb == 3 else 9)
        for n in (16, 301):
            assert _batch_label(dtype, nb, n, k) == s_label(dtype, k)
            _batch_exact(dtype, nb, n, k, res=nb != 13, out_f32=n == 301)
            _batch_random(dtype, nb, n, k, res=nb == 13, act=n == 16, out_f32=nb != 16)
            _batch_random(dtype, nb, n, k)


@pytest.mark.parametrize("dtype", BITS16)
def test_gemm_skinny_qkv_and_fallback(dtype, mfma_min):
    mfma_min(9)
    hist = [(5 * b + 2) % 6 for b in range(13)]
    hist[4] = 6
    for k in (256, 1280):                      # UNR 1 and 5; n = 768 and 3840
        _batch_random(dtype, 13, 3 * k, k, out_f32=False, hist=hist, S=6)
    assert _batch_label(dtype, 13, 301, 1352) == {b_label(dtype, 13, 301)}          # 1352 = 4 x 338: no 64-wide blocks per wave
    _batch_exact(dtype, 13, 301, 1352, True, True)
    _batch_random(dtype, 13, 301, 1352)


def _wide_against_skinny(dtype, nb, n, k, mfma_min, hist=None):
    """the wide kernel's column c is bit for bit column c % 16 of the 16-row kernel on sentences 16 (c / 16) ..."""
    mfma_min(9)
    got = _batch_random(dtype, nb, n, k, res=hist is None, out_f32=hist is None, hist=hist, S=6)
    if hist is not None:
        return
    _batch_exact(dtype, nb, n, k, True, False)
    w, _ = _weights(n, k, dtype)
    r = _rng(n, k, nb, 0)
    x = R.round_to(r.normal(0, 1, (nb, k)), dtype)
    bias, rs = _bias_res(r, k, (n,), (nb, n), True)
    mfma_min(1)
    for b0 in range(0, nb, 16):
        g = _launch(lambda: linear_batch(w, x[b0:b0 + 16], bias=bias, res=rs[b0:b0 + 16], dtype=dtype), s_label(dtype, k))["out"]
        m = min(16, nb - b0)
        assert np.array_equal(g[:m], got["out"][b0:b0 + m]), (dtype, nb, n, k, b0)


@pytest.mark.parametrize("nb", [17, 32, 33, 48, 49, 64])
@pytest.mark.parametrize("dtype", BITS16)
def test_gemm_skinny_wide(dtype, nb, mfma_min):
    """CT = 2, 3, 4 at both ends; N = 301: one tile per block (TR = 1) with a ragged tile; N = 16 cus + 5: two tiles per block;
    K = 2560: KS = 8, UNR = 5; K = 1280: UNR = 5 at KS = 4; and the QKV epilogue at both UNR"""
    _wide_against_skinny(dtype, nb, 301, 256, mfma_min)
    _wide_against_skinny(dtype, nb, 16 * _cus() + 5, 256, mfma_min)
    _wide_against_skinny(dtype, nb, 301, 2560, mfma_min)
    _wide_against_skinny(dtype, nb, 301, 1280, mfma_min)
    hist = [(5 * b + 2) % 6 for b in range(nb)]
    hist[nb - 1] = 6
    for k in (256, 1280):
        _wide_against_skinny(dtype, nb, 3 * k, k, mfma_min, hist=hist)


def test_every_reachable_instantiation_ran():
    """runs last (pytest keeps file order): the labels seen across the module are exactly the dispatch's reach"""
    want = reachable()
    assert SEEN, "the cases did not run"
    assert SEEN == want, (sorted(want - SEEN), sorted(SEEN - want))
