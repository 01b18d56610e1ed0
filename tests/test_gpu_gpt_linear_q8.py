"""GPU: the decode-step linear kernels of the IndexTTS GPT on per-channel uint8 weights (csrc/gpt_q8.hip gemv_d_q8_kernel,
gemv_b_q8_kernel, gemm_skinny_q8_kernel, gemm_skinny_wide_q8_kernel), one launch at a time through the unit entries
mi_gpt_linear_decode_q8 / mi_gpt_linear_batch_q8 (the engine's own launchers), against the float64 reference tests/gpt_q8_ref.py.
Activations are f16 (the only type a q8 handle takes).  The library profiler's kernel label of every launch says which instantiation
ran; the last test asserts that the file reached every q8 instantiation the dispatch can reach on this device.

Exact family (the forms without LayerNorm): q any bytes, zp any byte, scale a power of two, small-integer x / bias / res — every
sum is exact in fp32 in any order (gpt_q8_ref.py), so the result must be np.array_equal to the integer reference (fp32 output) or
to its rounding (f16 output).  No tolerance.

Random family: w std 0.05 quantised by weights.quantize_u8 (matrices above 2^20 elements: bytes drawn to the same picture, see
_weights), x std 1 rounded to f16, LayerNorm gains near 1.  Per element
|out - ref| <= G * 2^-24 * scale[n] * sum_k |(q - zp) x'|  (+ A_GELU * max(1, |v|) with the activation) (+ one unit in the last
place of an f16 output), the terms of tests/test_gpu_gpt_linear.py.  G per kernel family is MEASURED here, against the reference
alone, over this file's fp32-output cases without activation; the gate is twice the measured value rounded up to one digit.  Caps
that the gates must respect whatever was measured (asserted per case): G <= K / 64 + 12 on the VALU kernels, G <= K / (8 KS) + 12
on the matrix-core kernels, A_GELU <= 2e-5.

Measured on an MI355X (256 CUs; printed at the end of a run with -s), and the gates that follow:

    family                                    measured G   gate
    gemv_d_q8 plain            d_plain          0.687        2
    gemv_d_q8 LayerNorm        d_ln             2.665        6
    gemv_d_q8 LN + leading LN  d_pre            0.405        0.9
    gemv_b_q8                  gemv_b           1.830        4
    gemm_skinny(_wide)_q8      mfma             1.169        3
    A_GELU                                      1.448e-6     3e-6

Every gate is below the smallest cap of its family (12.25 at K = 16).  Wall time of the file: 7 s for its 50 tests.
A ragged K ends 48 elements (three 16-byte lanes) into the last 64-lane iteration.
"""
import functools

import numpy as np
import pytest

import gpt_linear_ref as R
import gpt_q8_ref as Q
from mi355tts import _lib
from mi355tts import weights as W
from mi355tts.indextts import linear_batch, linear_decode

pytestmark = pytest.mark.gpu

DT = "f16"
TL = "_Float16"
NAN = np.float32(np.nan)
# gate = 2 x measured, one digit up (module docstring); family -> G
GATE = {"d_plain": 2.0, "d_ln": 6.0, "d_pre": 0.9, "gemv_b": 4.0, "mfma": 3.0}
A_GELU = 3e-6
MEASURED_G, MEASURED_A, SEEN = {}, [0.0], set()
KI_PLAIN = [1, 2, 3, 4, 5, 6, 8]
KI_LN = [1, 2, 3, 4]
PER = 1024                     # elements of K per iteration of a wave: 64 lanes x 16 bytes


# ---------------------------------------------------------------------------------------------------------------
# the dispatch rules of csrc/gpt_q8.hip, restated
# ---------------------------------------------------------------------------------------------------------------
def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ki(k, ln):
    ki = -(-k // PER)
    return next(t for t in (KI_LN if ln else KI_PLAIN) if t >= ki)


def _r_ln(n, qkv):
    r = 1
    while r < (2 if qkv else 5) and -(-n // (8 * r)) > _cus():
        r += 1
    return r


def _b(v):
    return "true" if v else "false"


def d_label(k, n, ln=False, qkv=False):
    return f"gemv_d_q8_kernel<{TL}, {_r_ln(n, qkv) if ln else 1}, {_ki(k, ln)}, {8 if ln else 4}, {_b(ln)}, {_b(qkv)}>"


def b_label(nb, n, qkv=False):
    bb = 2 if nb <= 2 else 4 if nb <= 4 else 8 if nb <= 8 else 16
    return f"gemv_b_q8_kernel<{TL}, {2 if n >= 4096 else 1}, {bb}, {_b(qkv)}>"


def _ks(k):
    return 8 if k > 2048 else 4


def _unr(k):
    return 5 if (k // _ks(k)) % 320 == 0 else 1


def s_label(k, qkv=False):
    return f"gemm_skinny_q8_kernel<{TL}, {_b(qkv)}, {_unr(k)}>"


def w_label(k, nb, qkv=False):
    return f"gemm_skinny_wide_q8_kernel<{TL}, {_b(qkv)}, {_unr(k)}, {-(-nb // 16)}>"


def _qkv_ks(ki):
    return [k for k in range(64, PER * KI_LN[-1] + 1, 64) if _ki(k, True) == ki]


def _qkv_r_reachable(ki):
    return sorted({_r_ln(3 * k, True) for k in _qkv_ks(ki)})


def _qkv_k(ki, r):
    return next(k for k in _qkv_ks(ki) if _r_ln(3 * k, True) == r)


def reachable():
    s = {f"gemv_d_q8_kernel<{TL}, 1, {ki}, 4, false, false>" for ki in KI_PLAIN}
    for ki in KI_LN:
        s |= {f"gemv_d_q8_kernel<{TL}, {r}, {ki}, 8, true, false>" for r in range(1, 6)}
        s |= {f"gemv_d_q8_kernel<{TL}, {r}, {ki}, 8, true, true>" for r in _qkv_r_reachable(ki)}
    s |= {f"gemv_b_q8_kernel<{TL}, {r}, {bb}, {q}>" for r in (1, 2) for bb in (2, 4, 8, 16) for q in ("true", "false")}
    s |= {f"gemm_skinny_q8_kernel<{TL}, {q}, {u}>" for q in ("true", "false") for u in (1, 5)}
    s |= {f"gemm_skinny_wide_q8_kernel<{TL}, {q}, {u}, {ct}>" for q in ("true", "false") for u in (1, 5) for ct in (2, 3, 4)}
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
        print("\ngpt q8 linear, measured G (worst |out - ref| / (2^-24 scale sum |(q - zp) x'|), fp32 output, no activation): "
              + ", ".join(f"{f} {MEASURED_G.get(f, 0.0):.3f}" for f in GATE) + f"; A_GELU {MEASURED_A[0]:.3e}")


@pytest.fixture
def mfma_min():
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
    return np.random.default_rng([9527, 8, *key])


@functools.lru_cache(maxsize=2)
def _weights(n, k):
    """(q, scale, zp) of (n, k) weights, std 0.05, and the float64 matrix they stand for.  Up to 2^20 elements: normal weights
    through weights.quantize_u8.  Above: the same picture drawn directly (bytes around the zero point with std 42, a pool of
    2^20 + 7 laid out cyclically; scale 0.05 / 42 within a factor 1.5; zp 100 .. 155), which spares the test the quantiser."""
    r = _rng(n, k)
    if n * k <= 1 << 20:
        q8 = W.quantize_u8(r.normal(0, 0.05, (n, k)).astype(np.float32))
    else:
        zp = r.integers(100, 156, n).astype(np.uint8)
        pool = r.normal(0, 42, (1 << 20) + 7)
        q = np.clip(np.rint(np.resize(pool, (n, k)) + zp[:, None]), 0, 255).astype(np.uint8)
        q8 = (q, (0.05 / 42 * r.uniform(1 / 1.5, 1.5, n)).astype(np.float32), zp)
    return q8, Q.weights64(*q8)


def _bias_res(r, k, bshape, rshape, res):
    """bias and residual at the scale of the sums (tests/test_gpu_gpt_linear.py); none at the smallest K"""
    if k <= 16:
        return None, None
    sc = 0.05 * np.sqrt(k)
    return r.normal(0, 0.5 * sc, bshape).astype(np.float32), (r.normal(0, sc, rshape).astype(np.float32) if res else None)


def _ln_vec(k, *key):
    r = _rng(k, *key)
    return (1 + r.normal(0, 0.1, k)).astype(np.float32), r.normal(0, 0.1, k).astype(np.float32)


def _cap(fam, k):
    return k / (8 * _ks(k)) + 12 if fam == "mfma" else k / 64 + 12


def _check(out, ref, fam, k, out_f32, act, what):
    assert GATE[fam] <= _cap(fam, k) and A_GELU <= 2e-5, "a gate exceeds its cap"
    want, base = ref["out"], 2.0 ** -24 * ref["mag"]
    assert out.shape == want.shape and np.isfinite(out).all(), (what, "non-finite output")
    err = np.abs(out.astype(np.float64) - want)
    amp = np.maximum(1.0, np.abs(ref["v"]))
    g = float((err / np.maximum(base, 1e-300)).max())
    if out_f32 and not act:
        MEASURED_G[fam] = max(MEASURED_G.get(fam, 0.0), g)
    if out_f32 and act:
        MEASURED_A[0] = max(MEASURED_A[0], float((err / amp).max()))
    bar = GATE[fam] * base + (A_GELU * amp if act else 0.0) + (0.0 if out_f32 else R.ulp_bar(want, DT))
    ratio = err / np.maximum(bar, 1e-300)
    worst = float(ratio.max())
    print(f"{what} {fam}: worst err / bar {worst:.3f}, err / (2^-24 mag) {g:.3f}")
    assert worst <= 1.0, (what, fam, worst, np.unravel_index(int(ratio.argmax()), ratio.shape))


def _sentinel(shape):
    i = np.arange(int(np.prod(shape)), dtype=np.int64)
    return (64.0 + ((i * 7) % 31) * 0.5).astype(np.float32).reshape(shape)


def _decode_case(n, k, *, ln=False, pre=False, act=False, res=False, out_f32=True, hist=None, S=6, key=0):
    q8, w64 = _weights(n, k)
    r = _rng(n, k, key)
    x = r.normal(0, 1, k).astype(np.float32)
    if pre:
        x = (2 * x + 0.5).astype(np.float32)
    if not ln:
        x = R.round_to(x, DT)
    bias, rs = _bias_res(r, k, (n,), (n,), res)
    lnv = _ln_vec(k, 1) if ln else None
    prev = _ln_vec(k, 2) if pre else None
    cache = (_sentinel((k // 64, S, 64)), _sentinel((k // 64, S, 64)) + 1) if hist is not None else None
    what = f"decode n={n} k={k} ln={ln} pre={pre} act={act} res={res} of={out_f32} hist={hist}"
    got = _launch(lambda: linear_decode(None, x, q8=q8, bias=bias, ln=lnv, pre=prev, res=rs, act=act, out_f32=out_f32, cache=cache,
                                        hist=hist or 0, dtype=DT), d_label(k, n, ln, hist is not None))
    ref = R.linear(w64, x, bias, rs, act, lnv, prev)
    fam = "d_pre" if pre else "d_ln" if ln else "d_plain"
    if pre:
        e = np.abs(got["pre_out"].astype(np.float64) - ref["pre_out"]).max()
        assert np.isfinite(got["pre_out"]).all() and e <= 2e-5 * np.abs(ref["pre_out"]).max(), (what, e)
    if hist is None:
        _check(got["out"], ref, fam, k, out_f32, act, what)
        return
    qp = {kk: ref[kk][:k] for kk in ("out", "mag", "v")}
    _check(got["out"][:k], qp, fam, k, out_f32, act, what + " q")
    assert np.isnan(got["out"][k:]).all(), (what, "the k / v thirds of out were written")
    for name, c0, lo in (("K", cache[0], k), ("V", cache[1], 2 * k)):
        c1 = got[name]
        rest = np.ones(c0.shape, bool)
        if hist < S:
            rest[:, hist] = False
            part = {kk: ref[kk][lo:lo + k].reshape(k // 64, 64) for kk in ("out", "mag", "v")}
            _check(c1[:, hist], part, fam, k, False, act, what + " " + name)
            assert (c1[:, hist] != c0[:, hist]).all(), (what, name, "row hist still holds the sentinel")
        assert np.array_equal(c1[rest], c0[rest]), (what, name, "a cache element outside row hist changed")


def _want(ref, out_f32):
    return ref.astype(np.float32) if out_f32 else R.round_to(ref, DT)


def _exact_decode(n, k, res, out_f32):
    q, scale, zp, x, bias, rs = Q.exact_case_q8(n, k, 1, with_res=res)
    got = _launch(lambda: linear_decode(None, x[0], q8=(q, scale, zp), bias=bias, res=rs[0] if res else None, out_f32=out_f32,
                                        dtype=DT), d_label(k, n))["out"]
    want = _want(Q.linear_q8(q, scale, zp, x[0], bias, rs[0] if res else None)["out"], out_f32)
    assert np.array_equal(got, want), (n, k, res, out_f32, np.flatnonzero(got != want)[:8])


# ---------------------------------------------------------------------------------------------------------------
# gemv_d_q8_kernel
# ---------------------------------------------------------------------------------------------------------------
def _two_k(ki):
    return [ki * PER, (ki - 1) * PER + 48]


@pytest.mark.parametrize("ki", KI_PLAIN)
def test_gemv_d_plain_every_ki(ki):
    """N = 37 (rows end inside a block), the full and a ragged K of every KI, with and without res, fp32 and f16 output"""
    for k in _two_k(ki):
        assert _ki(k, False) == ki
        for res in (False, True):
            for of in (True, False):
                _exact_decode(37, k, res, of)
                _decode_case(37, k, res=res, out_f32=of)


def test_gemv_d_plain_k16():
    for of in (True, False):
        for res in (False, True):
            _exact_decode(37, 16, res, of)
        _decode_case(37, 16, out_f32=of)
    _exact_decode(1, 16, True, True)


@pytest.mark.parametrize("ki", KI_LN)
def test_gemv_d_ln_every_ki_and_r(ki):
    """fused LayerNorm: R = 1 at N = 37 with the full and a ragged K, with the activation and both output types; then every
    R in 2 .. 5 at its smallest N, and the QKV form at every R it can have at this KI"""
    for k in _two_k(ki):
        assert _ki(k, True) == ki
        for act, of in ((False, True), (True, True), (True, False), (False, False)):
            _decode_case(37, k, ln=True, act=act, out_f32=of)
    k = _two_k(ki)[1]
    for r in range(2, 6):
        n = 8 * _cus() * (r - 1) + 8
        assert _r_ln(n, False) == r
        _decode_case(n, k, ln=True)
    for r in _qkv_r_reachable(ki):
        kq = _qkv_k(ki, r)
        _decode_case(3 * kq, kq, ln=True, out_f32=False, hist=2)


@pytest.mark.parametrize("r", [1, 2, 3, 4, 5])
def test_gemv_d_ln_both_sides_of_every_r_boundary(r):
    """KI = 1 (K = 48): the smallest and the largest N that run R rows per wave on this device"""
    for n in (8 * _cus() * (r - 1) + 8, 8 * _cus() * r):
        assert _r_ln(n, False) == r
        _decode_case(n, 48, ln=True, act=r % 2 == 1)


def test_gemv_d_indextts_1_5_shapes():
    """hidden 1280: the QKV layer, the MLP's first layer with gelu_new, the head behind ln_f and final_norm"""
    _decode_case(3840, 1280, ln=True, out_f32=False, hist=3)
    _decode_case(5120, 1280, ln=True, act=True, out_f32=False)
    _decode_case(8194, 1280, ln=True, pre=True)


@pytest.mark.parametrize("k", [320, 1280, 2048])
def test_gemv_d_leading_layernorm(k):
    _decode_case(37, k, ln=True, pre=True)
    _decode_case(37, k, ln=True, pre=True, act=True, out_f32=False)


@pytest.mark.parametrize("hist", [0, 5, 6])
@pytest.mark.parametrize("k", [128, 704])
def test_gemv_d_qkv_cache_row(k, hist):
    """R = 1 (k = 128) and R = 2 (k = 704, 11 heads), max_seq = 6: hist 0, max_seq - 1 and max_seq (nothing is written)"""
    _decode_case(3 * k, k, ln=True, out_f32=False, hist=hist, S=6)
    _decode_case(3 * k, k, ln=True, out_f32=True, hist=hist, S=6, key=1)


# ---------------------------------------------------------------------------------------------------------------
# gemv_b_q8_kernel and the matrix-core kernels
# ---------------------------------------------------------------------------------------------------------------
def _batch_label(nb, n, k, qkv=False):
    """what launch_gpt_gemv_b runs at the options in force"""
    if nb >= _lib.get_option("gpt_mfma_min") and k % (_ks(k) * 64) == 0:
        return s_label(k, qkv) if nb <= 16 else w_label(k, nb, qkv)
    return {b_label(min(16, nb - b0), n, qkv) for b0 in range(0, nb, 16)}


def _batch_fam(label):
    return "mfma" if isinstance(label, str) and label.startswith("gemm_skinny") else "gemv_b"


def _batch_inputs(nb, n, k, res, key=0):
    r = _rng(n, k, nb, key)
    x = R.round_to(r.normal(0, 1, (nb, k)), DT)
    bias, rs = _bias_res(r, k, (n,), (nb, n), res)
    return x, bias, rs


def _check_caches(got, cache, ref_out, ref, nb, k, hist, S, fam, act, what, exact=False):
    for name, c0, lo in (("K", cache[0], k), ("V", cache[1], 2 * k)):
        c1 = got[name]
        rest = np.ones(c0.shape, bool)
        for b in range(nb):
            if hist[b] < S:
                rest[b, :, hist[b]] = False
                if exact:
                    assert np.array_equal(c1[b, :, hist[b]], R.round_to(ref_out[b, lo:lo + k], DT).reshape(k // 64, 64)), (what, name, b)
                else:
                    part = {kk: ref[kk][b, lo:lo + k].reshape(k // 64, 64) for kk in ("out", "mag", "v")}
                    _check(c1[b, :, hist[b]], part, fam, k, False, act, what + f" {name} slot {b}")
                    assert (c1[b, :, hist[b]] != c0[b, :, hist[b]]).all()
        assert np.array_equal(c1[rest], c0[rest]), (what, name, "a cache element outside the slots' rows changed")


def _batch_random(nb, n, k, *, act=False, res=False, out_f32=True, hist=None, S=6, key=0):
    q8, w64 = _weights(n, k)
    x, bias, rs = _batch_inputs(nb, n, k, res, key)
    qkv = hist is not None
    cache = (_sentinel((nb, k // 64, S, 64)), _sentinel((nb, k // 64, S, 64)) + 1) if qkv else None
    label = _batch_label(nb, n, k, qkv)
    fam = _batch_fam(label)
    what = f"batch nb={nb} n={n} k={k} act={act} res={res} of={out_f32} hist={hist}"
    got = _launch(lambda: linear_batch(None, x, q8=q8, bias=bias, res=rs, act=act, out_f32=out_f32, cache=cache, hist=hist,
                                       x_dead=np.full(k, NAN), dtype=DT), label)
    ref = R.linear(w64, x, bias, rs, act)
    assert np.isnan(got["out"][nb:]).all(), (what, "a row at or beyond nb was written")
    if not qkv:
        _check(got["out"][:nb], ref, fam, k, out_f32, act, what)
        return got
    _check(got["out"][:nb, :k], {kk: ref[kk][:, :k] for kk in ("out", "mag", "v")}, fam, k, out_f32, act, what + " q")
    assert np.isnan(got["out"][:nb, k:]).all(), (what, "the k / v thirds of out were written")
    _check_caches(got, cache, None, ref, nb, k, hist, S, fam, act, what)
    return got


def _batch_exact(nb, n, k, res, out_f32, hist=None, S=6):
    q, scale, zp, x, bias, rs = Q.exact_case_q8(n, k, nb, with_res=res)
    qkv = hist is not None
    cache = (_sentinel((nb, k // 64, S, 64)), _sentinel((nb, k // 64, S, 64)) + 1) if qkv else None
    got = _launch(lambda: linear_batch(None, x, q8=(q, scale, zp), bias=bias, res=rs, out_f32=out_f32, cache=cache, hist=hist,
                                       x_dead=np.full(k, NAN), dtype=DT), _batch_label(nb, n, k, qkv))
    ref = Q.linear_q8(q, scale, zp, x, bias, rs)["out"]
    cols = k if qkv else n
    want = _want(ref[:, :cols], out_f32)
    what = ("exact", nb, n, k, res, out_f32, hist)
    assert np.array_equal(got["out"][:nb, :cols], want), (what, np.argwhere(got["out"][:nb, :cols] != want)[:8])
    assert np.isnan(got["out"][nb:]).all() and np.isnan(got["out"][:nb, cols:]).all(), what
    if qkv:
        _check_caches(got, cache, ref, None, nb, k, hist, S, None, False, str(what), exact=True)
    return got


NB_B = [1, 2, 3, 5, 8, 9, 16]
K_B = [16, 1008, 1024, 1040, 2064]


@pytest.mark.parametrize("nb", NB_B)
def test_gemv_b_every_width_and_chunk_tail(nb, mfma_min):
    """N = 37 (R = 1) at every K: below a chunk, a chunk's tail, the exact chunk, just past it, two chunks and a ragged tail;
    N = 4101 (R = 2) at K = 16 and 2064.  x rows at and beyond nb are NaN."""
    mfma_min(65)
    for n, ks in ((37, K_B), (4101, [16, 2064])):
        for i, k in enumerate(ks):
            _batch_exact(nb, n, k, res=i % 2 == 0, out_f32=i % 3 != 0)
            _batch_random(nb, n, k, res=i % 2 == 1, out_f32=True)
            _batch_random(nb, n, k, act=True, out_f32=i % 2 == 0)


@pytest.mark.parametrize("nb", [2, 3, 5, 9])
def test_gemv_b_qkv_per_slot_rows(nb, mfma_min):
    """R = 1 (k = 128) and R = 2 (k = 1408, n = 4224): every slot its own hist — 0, max_seq - 1 and max_seq among them"""
    mfma_min(65)
    hist = [(3 * b + 5) % 6 for b in range(nb)]
    hist[0], hist[nb // 2], hist[nb - 1] = 0, 6, 5
    for k in (128, 1408):
        _batch_random(nb, 3 * k, k, out_f32=False, hist=hist, S=6)
    _batch_exact(nb, 384, 128, True, False, hist=hist)


def test_gemv_b_groups_of_16_where_k_does_not_split(mfma_min):
    """K = 1040 (no 64-wide blocks per wave) above 16 rows walks groups of 16 through gemv_b_q8_kernel"""
    mfma_min(9)
    for nb in (17, 40):
        assert _batch_label(nb, 37, 1040) == {b_label(16, 37), b_label(min(16, nb % 16), 37)}
        _batch_exact(nb, 37, 1040, True, True)
        _batch_random(nb, 37, 1040, res=True)


K_S = [256, 1280, 2560, 4096]


@pytest.mark.parametrize("k", K_S)
def test_gemm_skinny(k, mfma_min):
    """KS = 4 at K = 256 (one block per trip) and 1280 (five), KS = 8 at 2560 (five) and 4096 (one); N = 16 (one tile) and 301
    (ragged last tile); 9, 13 and 16 rows, and 3 rows with the threshold lowered"""
    for nb in (9, 13, 16, 3):
        mfma_min(2 if nb == 3 else 9)
        for n in (16, 301):
            assert _batch_label(nb, n, k) == s_label(k)
            _batch_exact(nb, n, k, res=nb != 13, out_f32=n == 301)
            _batch_random(nb, n, k, res=nb == 13, act=n == 16, out_f32=nb != 16)
            _batch_random(nb, n, k)


def test_gemm_skinny_qkv_and_fallback(mfma_min):
    mfma_min(9)
    hist = [(5 * b + 2) % 6 for b in range(13)]
    hist[0], hist[4], hist[12] = 0, 6, 5
    for k in (256, 1280):                      # UNR 1 and 5; n = 768 and 3840
        _batch_random(13, 3 * k, k, out_f32=False, hist=hist, S=6)
    _batch_exact(13, 768, 256, True, False, hist=hist)
    assert _batch_label(13, 301, 1360) == {b_label(13, 301)}          # 1360 = 4 x 340: no 64-wide blocks per wave
    _batch_exact(13, 301, 1360, True, True)
    _batch_random(13, 301, 1360)


def _wide_against_skinny(nb, n, k, mfma_min, hist=None):
    """the wide kernel's column c is bit for bit column c % 16 of the 16-row kernel on sentences 16 (c / 16) ..."""
    mfma_min(9)
    got = _batch_random(nb, n, k, res=hist is None, out_f32=hist is None, hist=hist, S=6)
    if hist is not None:
        return
    _batch_exact(nb, n, k, True, False)
    q8, _ = _weights(n, k)
    x, bias, rs = _batch_inputs(nb, n, k, True)
    mfma_min(1)
    for b0 in range(0, nb, 16):
        g = _launch(lambda: linear_batch(None, x[b0:b0 + 16], q8=q8, bias=bias, res=rs[b0:b0 + 16], dtype=DT), s_label(k))["out"]
        m = min(16, nb - b0)
        assert np.array_equal(g[:m], got["out"][b0:b0 + m]), (nb, n, k, b0)


@pytest.mark.parametrize("nb", [17, 33, 48, 64])
def test_gemm_skinny_wide(nb, mfma_min):
    """CT = 2, 3, 4; N = 301: one tile per block (TR = 1) with a ragged tile; N = 16 cus + 5: two tiles per block; K = 2560:
    KS = 8, UNR = 5; K = 4096: KS = 8, UNR = 1; K = 1280: UNR = 5 at KS = 4; and the QKV epilogue at both UNR"""
    _wide_against_skinny(nb, 301, 256, mfma_min)
    _wide_against_skinny(nb, 16 * _cus() + 5, 256, mfma_min)
    _wide_against_skinny(nb, 301, 2560, mfma_min)
    _wide_against_skinny(nb, 301, 4096, mfma_min)
    _wide_against_skinny(nb, 301, 1280, mfma_min)
    hist = [(5 * b + 2) % 6 for b in range(nb)]
    hist[0], hist[1], hist[nb - 1] = 0, 5, 6
    for k in (256, 1280):
        _wide_against_skinny(nb, 3 * k, k, mfma_min, hist=hist)
    mfma_min(9)
    _batch_exact(nb, 768, 256, True, False, hist=hist)


def _refused(fn, text):
    with pytest.raises(_lib.MiError, match=text):
        fn()


def test_bad_arguments_are_refused_and_the_next_call_works():
    z = lambda *s: np.zeros(s, np.float32)
    q8 = lambda n, k: (np.zeros((n, k), np.uint8), np.ones(n, np.float32), np.zeros(n, np.uint8))
    ln = lambda k: (z(k) + 1, z(k))
    _refused(lambda: linear_decode(None, z(24), q8=q8(8, 24), dtype=DT), "multiple of 16")
    _refused(lambda: linear_batch(None, z(2, 24), q8=q8(8, 24), dtype=DT), "multiple of 16")
    _refused(lambda: linear_decode(None, z(32), q8=q8(8, 32), dtype="bf16"), "MI_F16")
    _refused(lambda: linear_batch(None, z(2, 32), q8=q8(8, 32), dtype="f32"), "MI_F16")
    _refused(lambda: linear_decode(None, z(4112), q8=q8(8, 4112), ln=ln(4112), dtype=DT), "fused LayerNorm supports K <= 4096")
    _refused(lambda: linear_decode(None, z(2064), q8=q8(8, 2064), ln=ln(2064), pre=ln(2064), dtype=DT), "LayerNorm supports K <= 2048")
    _refused(lambda: linear_decode(None, z(8208), q8=q8(8, 8208), dtype=DT), "K <= 8192")
    _refused(lambda: linear_decode(None, z(64), q8=q8(8, 64), ln=ln(64), res=z(8), dtype=DT), "no residual")
    with pytest.raises(ValueError):
        linear_decode(z(8, 32), z(32), q8=q8(8, 32), dtype=DT)
    _exact_decode(37, 80, True, True)
    _decode_case(37, 4096, ln=True)            # the widest row the LayerNorm form holds


def test_every_reachable_instantiation_ran():
    """runs last (pytest keeps file order): the labels seen across the module are exactly the dispatch's reach"""
    want = reachable()
    assert SEEN, "the cases did not run"
    assert SEEN == want, (sorted(want - SEEN), sorted(SEEN - want))
