"""GPU: the four attention launches of the IndexTTS GPT (csrc/gpt_attn.h: gpt_attn1_body under gpt_attn1_kernel and
gpt_attn1_beam_kernel, gpt_prompt_attn_body under gpt_attn_kernel and gpt_attn_packed_kernel), one launch at a time through the
unit entries mi_gpt_attn_* (the engine's own launchers), against the float64 reference tests/gpt_attention_ref.py.

Shape: 2 heads, max_seq = 704, f32 / f16 / bf16.  In the decode body wave 0 then makes three trips (key bases 0, 256, 512: both
halves of the double buffer and the return to the first), wave 3 two (192, 448), the last pass starts at 640, 704 is no multiple
of 256 and the second head exercises the head stride.

Bars (derived, not tuned).  |out - ref| <= 3e-5 * max(1, max |V|) — the project's fp32 bar for its fused kernels — plus, for
the 16-bit types, one unit in the last place of the output type at |ref| (2^-10 |ref| for f16, 2^-7 |ref| for bf16).  The
reference is evaluated on the inputs AFTER they were rounded to the type under test (values below 2^-14 flushed to zero), so
what is measured is the kernel's own fp32 arithmetic, __expf and the output rounding.  General scores are kept within |s| <= 16
(a q head whose scores exceed that is halved, which is exact); larger scores come from a one-hot q and are exact.

Inputs: (a) random, q std 1, K std 0.5, V std 0.6; (b) ramps of the score over the key index from a one-hot q, rising by 1 in
every 64-key pass (the running maximum moves in every pass: the `corr` rescale) or falling (the first pass fixes it; the merge
factors between waves do the work); (c) a needle: one key scores 40 above the rest, the output must be that key's value row, and
V carries the row index in columns 0 and 1 as (j & 31) / 32 and (j >> 5) / 32 — exact in bf16 — so a wrong row names itself.

Every cache row a launch must not read is NaN: rows >= kv, rows >= rows_g of a packed slot, for the beam launch every slot's
row at a position where no hypothesis' table names that slot (the table of the other parity names exactly such rows where the
group has one) and the prompt positions of every slot but the group's first.  A read of any of them makes the output NaN
whatever the weight.  The entries preset the output to NaN as well, so a row that is not written shows.

Measured on an MI355X, worst |out - ref| / bar over the whole file (printed at the end of a run with -s): f32 0.043, f16 0.460,
bf16 0.492 — the 16-bit figures are the output rounding, half a unit in the last place against a bar of one.  Wall time of the
file: 5.4 s for its 85 tests, the slowest (the needle sweep, 11 launches of 64 slots) 0.35 s.
"""
import numpy as np
import pytest

import gpt_attention_ref as R
from mi355tts import _lib
from mi355tts.indextts import attention_decode, attention_decode_beam, attention_prompt, attention_prompt_packed

pytestmark = pytest.mark.gpu

H, S, HID = 2, 704, 128
DTYPES = ["f32", "f16", "bf16"]
NAN = np.float32(np.nan)
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\ngpt attention, worst |out - ref| / bar: " + ", ".join(f"{d} {WORST.get(d, 0.0):.3f}" for d in DTYPES))


def _check(out, ref, V, dtype, what):
    """every element finite and within the bar; V = the values the launch may read (NaN elsewhere)"""
    assert out.shape == ref.shape and np.isfinite(out).all(), (what, "non-finite output: a stale row was read or a row not written")
    bar = 3e-5 * max(1.0, float(np.nanmax(np.abs(V)))) + R.ulp_bar(ref, dtype)
    ratio = np.abs(out.astype(np.float64) - ref) / bar
    worst = float(ratio.max())
    WORST[dtype] = max(WORST.get(dtype, 0.0), worst)
    print(f"{what} [{dtype}]: worst err / bar {worst:.3f}")
    assert worst <= 1.0, (what, dtype, worst, np.unravel_index(int(ratio.argmax()), ratio.shape))


def _rng(*key):
    return np.random.default_rng([9527, *key])


def _tame(q, s):
    """halve (exactly) every (row, head) of q whose largest |score| exceeds 16; s (rows, H, keys) with NaN where no key is"""
    big = np.nanmax(np.abs(s), axis=-1) > 16.0
    q = q.reshape(q.shape[0], H, 64) * np.where(big, np.float32(0.5), np.float32(1.0))[:, :, None]
    return np.ascontiguousarray(q.reshape(q.shape[0], HID), np.float32)


def _random_slots(ns, dtype, *key):
    rng = _rng(*key)
    q = R.round_to(rng.normal(0, 1.0, (ns, HID)), dtype)
    K = R.round_to(rng.normal(0, 0.5, (ns, H, S, 64)), dtype)
    V = R.round_to(rng.normal(0, 0.6, (ns, H, S, 64)), dtype)
    return q, K, V


def _poison_tail(K, V, kv):
    for r, n in enumerate(kv):
        K[r, :, n:] = NAN
        V[r, :, n:] = NAN


def _one_hot(ns, value=1.0):
    q = np.zeros((ns, HID), np.float32)
    q[:, 0::64] = value                          # column 0 of every head
    return q


# ---------------------------------------------------------------------------------------------------------------
# decode, own slot
# ---------------------------------------------------------------------------------------------------------------
KVS = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 319, 320, 321, 511, 512, 513, 575, 576, 577, 640, 641, 703, 704]


def _decode_inputs(kind, kv, dtype):
    ns = len(kv)
    q, K, V = _random_slots(ns, dtype, 1, ns)
    if kind != "random":                         # the score of key j is K[j, 0] alone; the other K columns meet q = 0
        q = _one_hot(ns)
        step = np.arange(S) // 8
        ramp = (step if kind == "ramp_up" else step.max() - step) / 8.0          # 0 .. 10.875 in steps of 1/8: exact in bf16
        K[:, :, :, 0] = ramp.astype(np.float32)
    _poison_tail(K, V, kv)
    if kind == "random":
        q = _tame(q, np.einsum("nhd,nhjd->nhj", q.reshape(ns, H, 64), K))
    return q, K, V


@pytest.mark.parametrize("kind", ["random", "ramp_up", "ramp_down"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_every_pass_boundary(dtype, kind):
    """one launch, one slot per key count: around every multiple of 64 that starts a wave's first, second or third pass, and the
    last slot with hist = max_seq (kv clamped to 704)"""
    hist = [n - 1 for n in KVS] + [S]
    kv = KVS + [S]
    q, K, V = _decode_inputs(kind, kv, dtype)
    out = attention_decode(q, K, V, hist, dtype=dtype)
    _check(out, R.decode(q, K, V, kv), V, dtype, f"decode {kind}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_batched_mixed_lengths(dtype):
    """slots whose waves 1-3 have no key beside full ones"""
    kv = [1, 300, 704, 65]
    for kind in ("random", "ramp_up"):
        q, K, V = _decode_inputs(kind, kv, dtype)
        out = attention_decode(q, K, V, [n - 1 for n in kv], dtype=dtype)
        _check(out, R.decode(q, K, V, kv), V, dtype, f"decode mixed {kind}")


_BASE = {}


def _needle_base(dtype):
    if dtype not in _BASE:
        _, K, V = _random_slots(64, dtype, 2)
        K[:, :, :, 0] = 0.0
        j = np.arange(S)
        V[:, :, :, 0] = ((j & 31) / 32.0).astype(np.float32)
        V[:, :, :, 1] = ((j >> 5) / 32.0).astype(np.float32)
        _BASE[dtype] = (K, V)
    return _BASE[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_needle_at_every_position(dtype):
    """the needle at every key position 0 .. 703 (64 slots a launch, 11 launches); even slots hold 704 keys, odd slots end at
    their needle; head 1's needle sits elsewhere ((5 j) mod kv)"""
    K0, V0 = _needle_base(dtype)
    q = _one_hot(64)
    for first in range(0, S, 64):
        K, V = K0.copy(), V0.copy()
        pos = np.arange(first, first + 64)
        kv = np.where(np.arange(64) % 2 == 0, S, pos + 1)
        pos1 = (5 * pos) % kv
        K[np.arange(64), 0, pos, 0] = 40.0
        K[np.arange(64), 1, pos1, 0] = 40.0
        _poison_tail(K, V, kv)
        out = attention_decode(q, K, V, kv - 1, dtype=dtype)
        got = np.rint(out[:, [0, 64]] * 32) + 32 * np.rint(out[:, [1, 65]] * 32)          # the row each head fetched
        assert np.isfinite(out).all() and np.array_equal(got, np.stack([pos, pos1], 1)), \
            ("rows fetched (head 0, head 1) / wanted", got.tolist(), np.stack([pos, pos1], 1).tolist())
        _check(out, R.decode(q, K, V, kv), V, dtype, f"decode needle {first}..{first + 63}")


# ---------------------------------------------------------------------------------------------------------------
# decode, beam
# ---------------------------------------------------------------------------------------------------------------
# P -> ndec of the first hypothesis of group 0 (odd) and of group 1 (even); hypothesis i of a group has 2 i selections fewer
BEAM_NDEC = {1: (703, 300), 70: (259, 634), 300: (403, 404)}


def _beam_case(dtype, beams, P):
    ns = 2 * beams
    rng = _rng(3, beams, P)
    q, Kr, Vr = _random_slots(ns, dtype, 4, beams, P)
    hist = np.zeros(ns, np.int32)
    ndec = np.zeros(ns, np.int32)
    anc = rng.integers(0, beams, (2, ns, S)).astype(np.int32)
    K = np.full(Kr.shape, NAN, np.float32)
    V = np.full(Vr.shape, NAN, np.float32)
    nlive = max(1, beams // 2)
    for g in range(2):
        s0 = g * beams
        K[s0, :, :P], V[s0, :, :P] = Kr[s0, :, :P], Vr[s0, :, :P]        # the prompt's rows: in the group's first slot only
        top = BEAM_NDEC[P][g]
        side = top & 1
        order = np.argsort(rng.random((top, beams)), axis=1)             # per position: the slots hypotheses may name, then the rest
        live, dead = order[:, :nlive], order[:, nlive:]
        for i in range(beams):
            s = s0 + i
            ndec[s] = top - 2 * i
            hist[s] = P + ndec[s] - 1
            n = np.arange(ndec[s])
            anc[side, s, n] = live[n, rng.integers(0, nlive, n.size)]
            if beams > 1:                                                # the other parity's table names rows that are NaN
                anc[1 - side, s, n] = dead[n, rng.integers(0, beams - nlive, n.size)]
        n = np.arange(top)
        for c in range(nlive):
            K[s0 + live[:, c], :, P + n] = Kr[s0 + live[:, c], :, P + n]
            V[s0 + live[:, c], :, P + n] = Vr[s0 + live[:, c], :, P + n]
    assert hist.max() + 1 == S and {int(x) & 1 for x in ndec} == {0, 1}
    Kp, Vp, kv = R.beam_gather(K, V, hist, ndec, beams, anc)
    q = _tame(q, np.einsum("nhd,nhjd->nhj", q.reshape(ns, H, 64), Kp))
    return q, K, V, hist, ndec, anc, Kp, Vp, kv


@pytest.mark.parametrize("P", [1, 70, 300])
@pytest.mark.parametrize("beams", [1, 3, 8])
@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_beam_through_the_ancestor_table(dtype, beams, P):
    """two groups (the second group's first slot is not slot 0), odd and even ndec, up to 704 keys found through the table"""
    q, K, V, hist, ndec, anc, Kp, Vp, kv = _beam_case(dtype, beams, P)
    out = attention_decode_beam(q, K, V, hist, ndec, anc, beams=beams, dtype=dtype)
    _check(out, R.decode(q, Kp, Vp, kv), Vp, dtype, f"beam B={beams} P={P}")
    if dtype == "f32":        # gpt_beam.hip: on a privately owned cache the own-slot kernel gives the same bits
        np.testing.assert_array_equal(out, attention_decode(q, Kp, Vp, hist, dtype=dtype))


# ---------------------------------------------------------------------------------------------------------------
# prompt, lone
# ---------------------------------------------------------------------------------------------------------------
def _prompt_case(dtype, hist, rows, *key):
    rng = _rng(5, hist, rows, *key)
    n = hist + rows
    q = R.round_to(rng.normal(0, 1.0, (rows, HID)), dtype)
    K = R.round_to(rng.normal(0, 0.5, (H, S, 64)), dtype)
    V = R.round_to(rng.normal(0, 0.6, (H, S, 64)), dtype)
    K[:, n:] = NAN
    V[:, n:] = NAN
    q = _tame(q, np.einsum("rhd,hjd->rhj", q.reshape(rows, H, 64), K[:, :n]))
    return q, K, V


@pytest.mark.parametrize("rows", [1, 8, 9, 63, 64, 65, 511, 512, 513, 704])
@pytest.mark.parametrize("dtype", DTYPES)
def test_prompt_lone_every_row(dtype, rows):
    """history 0, mask on, every row compared: the 8-keys-per-wave value pass (8, 9), the wave (63 .. 65) and the 512-thread
    strided key loop coming round (511 .. 513, 704)"""
    q, K, V = _prompt_case(dtype, 0, rows)
    out = attention_prompt(q, K, V, 0, flag=1, dtype=dtype)
    _check(out, R.prompt(q, K, V, 0, rows, 1), V, dtype, f"prompt rows={rows}")


@pytest.mark.parametrize("flag", [1, 0])
@pytest.mark.parametrize("dtype", DTYPES)
def test_prompt_lone_with_history(dtype, flag):
    """history 5, 75 new rows: the mask's row index is the position inside the new block (oracle/gpt_np.py:93-96), so with the
    mask on row i sees keys 0 .. i of the 80, not 0 .. 5 + i"""
    q, K, V = _prompt_case(dtype, 5, 75, flag)
    out = attention_prompt(q, K, V, 5, flag=flag, dtype=dtype)
    _check(out, R.prompt(q, K, V, 5, 75, flag), V, dtype, f"prompt hist=5 rows=75 flag={flag}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_prompt_mask_is_an_added_minus_128(dtype):
    """one-hot q, exact scores: key 70 of 80 scores 125, every other key 0.  For the rows before it the mask leaves it at -3
    against the visible keys — a weight of e^-3 each row must still count (a kernel that skips masked keys, or uses -inf,
    loses up to 5 % of the output) — and for rows 70 .. 79 it is a needle 125 above the rest"""
    rows, f = 80, 70
    rng = _rng(6)
    q = _one_hot(rows)
    K = R.round_to(rng.normal(0, 0.5, (H, S, 64)), dtype)
    V = R.round_to(rng.normal(0, 0.6, (H, S, 64)), dtype)
    K[:, :, 0] = 0.0
    K[:, f, 0] = 125.0
    K[:, rows:] = NAN
    V[:, rows:] = NAN
    ref = R.prompt(q, K, V, 0, rows, 1)
    skipped = np.stack([R.prompt(q[i:i + 1], K, V, i, 1, 0)[0] for i in range(rows)])      # keys 0 .. i alone
    assert np.abs(ref - skipped)[:f].max() > 1e-2                                            # the case tells the two apart
    out = attention_prompt(q, K, V, 0, flag=1, dtype=dtype)
    _check(out, ref, V, dtype, "prompt -128")


# ---------------------------------------------------------------------------------------------------------------
# prompt, packed
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_prompt_packed_segments(dtype):
    """four prompts of 7, 530, 1 and 166 rows in slots 2, 0, 3, 1 (704 packed rows); no row beyond a segment's own is read"""
    seg_rows, slots = (7, 530, 1, 166), (2, 0, 3, 1)
    segs, first = [], 0
    for r, s in zip(seg_rows, slots):
        segs.append((first, r, s))
        first += r
    rng = _rng(7)
    q = R.round_to(rng.normal(0, 1.0, (first, HID)), dtype)
    K = R.round_to(rng.normal(0, 0.5, (4, H, S, 64)), dtype)
    V = R.round_to(rng.normal(0, 0.6, (4, H, S, 64)), dtype)
    for f0, r, s in segs:
        K[s, :, r:] = NAN
        V[s, :, r:] = NAN
        q[f0:f0 + r] = _tame(q[f0:f0 + r], np.einsum("rhd,hjd->rhj", q[f0:f0 + r].reshape(r, H, 64), K[s, :, :r]))
    out = attention_prompt_packed(q, K, V, segs, dtype=dtype)
    _check(out, R.prompt_packed(q, K, V, segs), V, dtype, "prompt packed")
    if dtype == "f32":        # the same body as the lone kernel: the same bits
        for f0, r, s in segs:
            np.testing.assert_array_equal(out[f0:f0 + r], attention_prompt(q[f0:f0 + r], K[s], V[s], 0, flag=1, dtype=dtype))


# ---------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_errors_and_the_next_call_works():
    q, K, V = _random_slots(4, "f32", 8)
    z = np.zeros((2, 4, S), np.int32)
    bad = [
        lambda: attention_decode(q, K, V, [0, 0, 0, S + 1]),                                       # hist beyond max_seq
        lambda: attention_decode(q, K, V, [0, -1, 0, 0]),
        lambda: attention_decode_beam(q, K, V, [5] * 4, [1] * 4, z, beams=0),
        lambda: attention_decode_beam(q, K, V, [5] * 4, [1] * 4, z, beams=3),                      # does not divide 4 slots
        lambda: attention_decode_beam(q, K, V, [5] * 4, [7] * 4, z, beams=2),                      # ndec > hist + 1
        lambda: attention_decode_beam(q, K, V, [5] * 4, [1] * 4, z + 2, beams=2),                  # table entry out of range
        lambda: attention_prompt(q, K[0], V[0], S - 3, flag=1),                                    # hist + rows > max_seq
        lambda: attention_prompt(q, K[0], V[0], 0, flag=2),
        lambda: attention_prompt_packed(q, K, V, [(0, 2, 0), (3, 1, 1)]),                          # a gap
        lambda: attention_prompt_packed(q, K, V, [(0, 2, 0), (2, 2, 0)]),                          # a slot twice
        lambda: attention_prompt_packed(q, K, V, [(0, 2, 0), (2, 1, 1)]),                          # 3 rows in the table, 4 in q
        lambda: attention_prompt_packed(q, K, V, [(0, 2, 0), (2, 2, 4)]),                          # no such slot
    ]
    for k, call in enumerate(bad):
        with pytest.raises(_lib.MiError, match="mi_gpt_attn"):
            call()
        assert len(_lib.load().mi_last_error()) > 20, k
    kv = [3, 1, S, 65]
    q, K, V = _decode_inputs("random", kv, "f32")
    out = attention_decode(q, K, V, [n - 1 for n in kv])
    _check(out, R.decode(q, K, V, kv), V, "f32", "decode after the errors")
