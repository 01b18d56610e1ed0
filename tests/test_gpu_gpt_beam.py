"""GPU: beam search of the IndexTTS GPT (csrc/gpt_beam.hip) against the float64 restatement of its definition
(tests/gpt_beam_ref.py): the unit entry on rows of logits, then the decode loop — one beam against the greedy entries, the device
beam against a host-driven beam over the engine's own single-sentence step (every hypothesis with a private copy of the cache:
what the ancestor table, the move between slots and the beam attention have to be indistinguishable from), against the numpy
oracle, and its invariances.

Scores hold to |d| <= 1e-5 + 2^-22 |score|; parents and tokens are compared wherever the reference's margin (the smallest gap
among the sorted top B + 1 candidates) is at least 4 x that, and the selections below it are counted."""
import numpy as np
import pytest

import gpt_beam_ref as R
from mi355tts import weights as W
from mi355tts import _lib
from mi355tts.config import IndexGPTConfig
from mi355tts.indextts import IndexGPT, Sampling, beam_select

pytestmark = pytest.mark.gpu
SEED = 9527
N_NEW = 24
MARGIN = 1e-4             # host-side margin from which a decode case is compared in full
KW = dict(repeat_value=0.7, penalty_range=3)


# ---------------------------------------------------------------------------------------------------------------
# 1: mi_gpt_beam_select
# ---------------------------------------------------------------------------------------------------------------
def test_beam_select_vs_reference():
    n = low = 0
    for codes in R.UNIT_CODES:
        for groups in R.UNIT_GROUPS:
            for beams in R.UNIT_BEAMS:
                lg, pen, prev = R.unit_case(codes, groups, beams)
                for first in (True, False):
                    par, tok, sc = beam_select(lg, prev, beams=beams, first=first, pen=pen)
                    rp, rt, rs, margins = R.unit_reference(lg, pen, prev, groups, beams, first)
                    for g in range(groups):
                        what = (codes, groups, beams, first, g)
                        t = R.tol(rs[g])
                        n += 1
                        if margins[g] < 4 * t.max():
                            low += 1
                            continue
                        assert par[g].tolist() == rp[g].tolist() and tok[g].tolist() == rt[g].tolist(), what
                        d = np.abs(sc[g].astype(np.float64) - rs[g])
                        assert (d <= t).all(), (what, float(d.max()))
    assert n == 160 and low <= n // 100, (n, low)


def test_beam_select_first_reads_one_row_per_group():
    lg, pen, prev = R.unit_case(1000, 3, 5)
    want = beam_select(lg, None, beams=5, first=True, pen=pen)
    bad_l, bad_p = lg.copy(), pen.copy()
    for g in range(3):
        bad_l[g * 5 + 1:(g + 1) * 5] = np.nan
        bad_p[g * 5 + 1:(g + 1) * 5] = np.nan
    got = beam_select(bad_l, np.full(15, np.nan, np.float32), beams=5, first=True, pen=bad_p)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    assert (want[0] == 0).all()


def test_beam_select_ties():
    """rows in steps of 0.25, identical rows and equal previous scores: exact ties inside and across rows go to the lower index"""
    for beams in (1, 2, 3, 5, 8):
        lg, prev = R.tie_rows(beams)
        for first in (True, False):
            par, tok, sc = beam_select(lg, prev, beams=beams, first=first)
            rp, rt, rs, _ = R.select(lg, None, prev, beams, first)
            assert par[0].tolist() == rp.tolist() and tok[0].tolist() == rt.tolist(), (beams, first)
            assert (np.abs(sc[0] - rs) <= R.tol(rs)).all()


def test_beam_select_errors_and_code_range():
    ok = np.zeros((2, 8), np.float32)
    pv = np.zeros(2, np.float32)
    for lg, kw in ((np.zeros((9, 16), np.float32), dict(beams=9)), (np.zeros((2, 1), np.float32), dict(beams=2)),
                   (np.zeros((1, 16385), np.float32), dict(beams=1))):
        with pytest.raises(_lib.MiError):
            beam_select(lg, np.zeros(lg.shape[0], np.float32), **kw)
    L = _lib.load()
    out = np.zeros(2, np.int32)
    sc = np.zeros(2, np.float32)
    assert L.mi_gpt_beam_select(ok.ctypes.data, None, pv.ctypes.data, 1, 0, 8, 0, out.ctypes.data, out.ctypes.data,
                                sc.ctypes.data, _lib.MI_HOST) != 0                       # beams < 1
    par, tok, s = beam_select(ok, pv, beams=2)                                           # the library is still usable
    assert tok[0].tolist() == [0, 1] and par[0].tolist() == [0, 0]
    par, tok, s = beam_select(np.full((1, 1), 3.0, np.float32), [-2.0], beams=1)          # one code: log-probability 0
    assert tok[0, 0] == 0 and par[0, 0] == 0 and s[0, 0] == -2.0
    lg, pen, prev = R.unit_case(16384, 1, 8)
    par, tok, s = beam_select(lg, prev, beams=8, pen=pen)
    rp, rt, rs, m = R.select(lg, pen, prev, 8, False)
    assert m < 4 * R.tol(rs).max() or (par[0].tolist() == rp.tolist() and tok[0].tolist() == rt.tolist())
    assert (np.abs(s[0] - rs) <= R.tol(rs)).all()


# ---------------------------------------------------------------------------------------------------------------
# 2-7: the decode loop
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    cfg = IndexGPTConfig.small()
    return cfg, W.synth_state(W.gpt_spec(cfg), SEED)


def _engine(small, max_batch, dtype="f32"):
    cfg0, st = small
    return IndexGPT(IndexGPTConfig(**{**cfg0.__dict__, "max_batch": max_batch}), st, dtype=dtype)


@pytest.fixture(scope="module")
def eng(small):
    e = _engine(small, 8)
    yield e
    e.close()


def _prompt(e, seed, n_text=6, n_cond=4):
    cfg = e.cfg
    conds = W.synth_normal(seed, "conds", (1, n_cond, cfg.hidden), std=0.5)
    text = (np.arange(n_text, dtype=np.int32) * 5 + seed) % (cfg.text_tokens - 2) + 2
    mh, _ = e.mel_embed(cfg.start_mel_token, 0)
    p, _ = e.concat(conds, e.text_embed(text), mh)
    return p


_HOST = {}


def _host_driven(e, seed, beams, stop_tokens=()):
    """the reference loop over the engine's own step, every hypothesis with its own copy of the cache; computed once per case"""
    key = (seed, beams, tuple(stop_tokens))
    if key not in _HOST:
        _HOST[key] = R.beam_generate(R.EngineModel(e), _prompt(e, seed), beams, N_NEW, stop_tokens=stop_tokens, **KW)
    return _HOST[key]


def _device(e, seed, beams, stop_tokens=(), max_new=N_NEW):
    res, pen = e.generate_beam([_prompt(e, seed)], [max_new], beams, stop_tokens=list(stop_tokens), **KW)
    return res[0], pen[0]


def _compare(dev, pen, ref, what):
    toks, hid, score = dev
    d = abs(score - ref["score"])
    print(f"beam {what}: min margin {min(ref['margins']):.3g}, score {score:.6f} (host-driven {ref['score']:.6f}, |d| {d:.3g}, "
          f"tolerance {R.tol(ref['score']):.3g}), max |d hidden| {np.abs(hid - ref['hidden'][: len(toks)]).max():.3g}")
    assert toks.tolist() == ref["tokens"], what
    assert d <= R.tol(ref["score"]), what
    np.testing.assert_allclose(hid, ref["hidden"], rtol=0, atol=2e-4)
    np.testing.assert_array_equal(pen, ref["pen"])                  # hypothesis 0's penalty vector, written back


def test_one_beam_is_greedy(eng):
    for seed in (1, 2):
        p = _prompt(eng, seed)
        ones = np.ones((1, eng.cfg.mel_codes), np.float32)
        t0, h0, p0 = eng.generate_from_prompt(p, N_NEW, stop_tokens=[], repeat_penality=ones, **KW)
        rb, pb = eng.generate_batch([p], [N_NEW], stop_tokens=[], **KW)
        (t1, h1, s1), p1 = _device(eng, seed, 1)
        assert len(t0) == N_NEW and t1.tolist() == t0.tolist() == rb[0][0].tolist()
        np.testing.assert_allclose(h1, h0, rtol=0, atol=2e-4)       # the batch-against-single bar of test_gpu_gpt.py
        np.testing.assert_allclose(h1, rb[0][1], rtol=0, atol=2e-4)
        np.testing.assert_array_equal(p1, pb[0])
        ref = _host_driven(eng, seed, 1)
        assert ref["tokens"] == t0.tolist() and abs(s1 - ref["score"]) <= R.tol(ref["score"])


# seeds 1-4 x beams 2-5; (seed 1, 4 beams) has a margin of 7.7e-5 at one selection (on the oracle's logits) and is replaced by the
# next seed by the same rule (seed 5, 4 beams: 4.0e-3)
CASES = [(5 if (s, b) == (1, 4) else s, b) for b in (2, 3, 4, 5) for s in (1, 2, 3, 4)]


@pytest.mark.parametrize("seed,beams", CASES)
def test_device_beam_vs_host_driven(eng, seed, beams):
    ref = _host_driven(eng, seed, beams)
    dev, pen = _device(eng, seed, beams)
    assert len(dev[0]) == N_NEW and len(ref["tokens"]) == N_NEW
    if min(ref["margins"]) < MARGIN:                                  # counted by test_enough_cases_are_compared
        print(f"beam ({seed}, {beams}): host-side margin {min(ref['margins']):.3g} below {MARGIN}, not compared")
        return
    _compare(dev, pen, ref, (seed, beams))


def test_enough_cases_are_compared(eng):
    full = sum(min(_host_driven(eng, s, b)["margins"]) >= MARGIN for s, b in CASES)
    assert len(CASES) == 16 and full >= 14, full


def test_device_beam_stops_with_hypothesis_0(eng):
    seed, beams = 2, 4
    free = _host_driven(eng, seed, beams)
    stop = free["top_tokens"][10]                                     # hypothesis 0's token after selection 10
    ref = _host_driven(eng, seed, beams, (stop, 1000))
    assert len(ref["tokens"]) == 11 and min(ref["margins"]) >= MARGIN
    dev, pen = _device(eng, seed, beams, (stop, 1000))
    assert len(dev[0]) == 11 and dev[1].shape == (11, eng.cfg.hidden)
    _compare(dev, pen, ref, (seed, beams, "stop"))


@pytest.mark.parametrize("seed,beams", [(3, 2), (3, 3)])
def test_device_beam_vs_oracle(eng, small, seed, beams):
    """smallest oracle-side margin of these two cases over the 24 selections: 7.7e-3, about six times the fp32 logits gate of
    test_medium_model_vs_oracle (4 x 3e-4)"""
    cfg, st = small
    ref = R.beam_generate(R.OracleModel(cfg, st), _prompt(eng, seed), beams, N_NEW, **KW)
    assert min(ref["margins"]) >= 6 * 4 * 3e-4
    (toks, hid, score), pen = _device(eng, seed, beams)
    gap = abs(score - ref["score"])
    if toks.tolist() != ref["tokens"]:
        k = next(i for i, (a, b) in enumerate(zip(toks.tolist(), ref["tokens"])) if a != b)
        print(f"beam vs oracle ({seed}, {beams}): first difference at step {k}, oracle margin there {ref['margins'][k]:.3g}, "
              f"engine-against-oracle score gap {gap:.3g}")
    assert toks.tolist() == ref["tokens"]
    print(f"beam vs oracle ({seed}, {beams}): score {score:.6f} / {ref['score']:.6f}, max |d hidden| "
          f"{np.abs(hid - ref['hidden']).max():.3g}")
    np.testing.assert_allclose(hid, ref["hidden"], rtol=0, atol=3e-4)
    np.testing.assert_array_equal(pen, ref["pen"])


def _equal(a, b):
    assert a[0].tolist() == b[0].tolist() and a[2] == b[2]           # tokens and score, bit for bit
    np.testing.assert_array_equal(a[1], b[1])


def test_groups_do_not_see_each_other(eng):
    p1, p2 = _prompt(eng, 1), _prompt(eng, 2, n_text=9)
    lim = [N_NEW, 17]
    both, pen = eng.generate_beam([p1, p2], lim, 3, stop_tokens=[], **KW)
    for g, p in enumerate((p1, p2)):
        alone, pa = eng.generate_beam([p], [lim[g]], 3, stop_tokens=[], **KW)
        assert len(alone[0][0]) == lim[g]
        _equal(both[g], alone[0])
        np.testing.assert_array_equal(pen[g], pa[0])
    twice, pen2 = eng.generate_beam([p1, p1], [N_NEW, N_NEW], 3, stop_tokens=[], **KW)       # first and second group
    _equal(twice[0], twice[1])
    _equal(twice[0], both[0])
    np.testing.assert_array_equal(pen2[0], pen2[1])


def test_graph_replay_equals_eager_beam(eng):
    p1, p2 = _prompt(eng, 3), _prompt(eng, 4)
    a, pa = eng.generate_beam([p1, p2], [N_NEW, N_NEW], 3, stop_tokens=[], **KW)
    a2, _ = eng.generate_beam([p1, p2], [N_NEW, N_NEW], 3, stop_tokens=[], **KW)             # the captured graph by now
    _lib.prof_reset(); _lib.prof_enable(("attn",))                                            # profiling: eager launches
    try:
        b, pb = eng.generate_beam([p1, p2], [N_NEW, N_NEW], 3, stop_tokens=[], **KW)
    finally:
        _lib.prof_enable(())
    for g in range(2):
        _equal(a[g], b[g])
        _equal(a[g], a2[g])
    np.testing.assert_array_equal(pa, pb)


def test_greedy_sampled_beam_on_one_handle(eng, small):
    p = _prompt(eng, 1)
    ones = np.ones((1, eng.cfg.mel_codes), np.float32)
    sp = Sampling(1.0, 30, 0.8, 31)

    def three(e):
        g = e.generate_from_prompt(p, N_NEW, stop_tokens=[], repeat_penality=ones, **KW)
        s = e.generate_from_prompt(p, N_NEW, stop_tokens=[], repeat_penality=ones, sampling=sp, **KW)
        b, _ = e.generate_beam([p], [N_NEW], 3, stop_tokens=[], **KW)
        gb, _ = e.generate_batch([p, p], [N_NEW, N_NEW], stop_tokens=[], **KW)
        return g, s, b[0], gb

    fresh = []
    for which in range(3):                       # what each call gives as the first call on a fresh handle
        e = _engine(small, 8)
        if which == 0:
            fresh.append(e.generate_from_prompt(p, N_NEW, stop_tokens=[], repeat_penality=ones, **KW))
        elif which == 1:
            fresh.append(e.generate_from_prompt(p, N_NEW, stop_tokens=[], repeat_penality=ones, sampling=sp, **KW))
        else:
            fresh.append(e.generate_beam([p], [N_NEW], 3, stop_tokens=[], **KW)[0][0])
        e.close()
    for _ in range(2):                           # interleaved, twice over, on the shared handle
        g, s, b, gb = three(eng)
        assert g[0].tolist() == fresh[0][0].tolist() and s[0].tolist() == fresh[1][0].tolist()
        np.testing.assert_array_equal(g[1], fresh[0][1])
        np.testing.assert_array_equal(s[1], fresh[1][1])
        _equal(b, fresh[2])
        assert gb[0][0].tolist() == gb[1][0].tolist() == g[0].tolist()
    # the drop-in step entry stays greedy after a beam call
    eng.reset()
    _, _, tok, lg = eng.step(p, ones, attention_mask=1, return_logits=True)
    assert int(tok[0, 0]) == int(np.argmax(lg)) == int(fresh[0][0][0])


# Beyond 64 keys.  Everything above runs at max_seq = 64: one 64-key pass in wave 0 of gpt_attn1_body.  Here the cache holds 352
# rows, so the ancestor lookup runs in all four waves, through both halves of a wave's double buffer (keys >= 256) and the merge.
@pytest.fixture(scope="module")
def long_eng(small):
    cfg = IndexGPTConfig(**{**small[0].__dict__, "max_seq": 352, "max_mel_pos": 352, "max_batch": 3})
    e = IndexGPT(cfg, W.synth_state(W.gpt_spec(cfg), SEED), dtype="f32")
    yield e
    e.close()


def test_one_beam_is_greedy_over_300_tokens(long_eng):
    """include/mi355tts.h: "num_beams == 1 is greedy exactly" — a 40-row prompt, 300 tokens, 339 keys at the end"""
    e = long_eng
    p = _prompt(e, 1, n_text=6, n_cond=31)
    assert p.shape[1] == 40
    rb, pb = e.generate_batch([p], [300], stop_tokens=[], **KW)
    res, p1 = e.generate_beam([p], [300], 1, stop_tokens=[], **KW)
    t1, h1, _ = res[0]
    assert len(t1) == 300 and t1.tolist() == rb[0][0].tolist()
    print(f"one beam, 300 tokens: max |d hidden| against generate_batch {np.abs(h1 - rb[0][1]).max():.3g}")
    # the same launches but for the attention, and in fp32 gpt_attn1_beam_kernel gives gpt_attn1_kernel's bits: equal rows
    np.testing.assert_array_equal(h1, rb[0][1])
    np.testing.assert_array_equal(p1[0], pb[0])


def test_device_beam_vs_host_driven_300_row_prompt(long_eng):
    """three beams over a 300-row prompt, 8 selections (P = 300: every later key is found through the table, in wave 0's and wave
    1's second pass), against the host-driven beam; the seed is the first of (1, 2, 3) whose host-side margin reaches MARGIN"""
    e = long_eng
    for seed in (1, 2, 3):
        p = _prompt(e, seed, n_text=6, n_cond=291)
        assert p.shape[1] == 300
        ref = R.beam_generate(R.EngineModel(e), p, 3, 8, stop_tokens=(), **KW)
        if min(ref["margins"]) >= MARGIN:
            break
        print(f"beam (300 rows, seed {seed}): host-side margin {min(ref['margins']):.3g} below {MARGIN}, next seed")
    assert min(ref["margins"]) >= MARGIN and len(ref["tokens"]) == 8
    res, pen = e.generate_beam([p], [8], 3, stop_tokens=[], **KW)
    assert len(res[0][0]) == 8
    _compare(res[0], pen[0], ref, (seed, 3, "300-row prompt"))


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_beam_16_bit_engines(small, dtype):
    e = _engine(small, 3, dtype)
    p = _prompt(e, 1)
    res, pen = e.generate_beam([p], [N_NEW], 3, stop_tokens=[], **KW)
    toks, hid, score = res[0]
    assert len(toks) == N_NEW and toks.min() >= 0 and toks.max() < e.cfg.mel_codes
    assert np.isfinite(hid).all() and np.isfinite(score) and score < 0.0
    one, _ = e.generate_beam([p], [N_NEW], 1, stop_tokens=[], **KW)
    gb, _ = e.generate_batch([p], [N_NEW], stop_tokens=[], **KW)
    assert one[0][0].tolist() == gb[0][0].tolist()
    e.close()


def test_beam_limits(eng):
    cfg = eng.cfg
    p = _prompt(eng, 1, n_text=18)                                   # P = 25: 25 + 40 - 1 == max_seq, 40 == max_mel_pos
    assert p.shape[1] + 40 - 1 == cfg.max_seq
    res, _ = eng.generate_beam([p], [40], 2, stop_tokens=[], **KW)
    assert len(res[0][0]) == 40
    with pytest.raises(_lib.MiError):
        eng.generate_beam([_prompt(eng, 1, n_text=19)], [40], 2, stop_tokens=[], **KW)       # one row more than the cache holds
    with pytest.raises(ValueError):
        eng.generate_beam([p, p, p], [4, 4, 4], 3, stop_tokens=[])                             # 9 slots, max_batch 8
    # the C entry's own checks: MI_EINVAL and the handle still decodes
    L = _lib.load()
    p1 = _prompt(eng, 1)
    cat = np.ascontiguousarray(np.concatenate([p1[0]] * 3, 0))
    rows = np.array([p1.shape[1]] * 3, np.int32)
    mx = np.array([4] * 3, np.int32)
    n = np.zeros(3, np.int32)
    toks = np.zeros((3, 4), np.int32)
    hid = np.zeros((3, 4, cfg.hidden), np.float32)
    for nb, beams in ((3, 3), (1, 0), (1, 9)):
        rc = L.mi_gpt_generate_beam(eng._h, nb, cat.ctypes.data, _lib.i32p(rows), _lib.i32p(mx), None, 0, 0.7, 3, None, beams,
                                    toks.ctypes.data, hid.ctypes.data, 4, _lib.i32p(n), None, _lib.MI_HOST)
        assert rc != 0, (nb, beams)
    again, _ = eng.generate_beam([p1], [N_NEW], 3, stop_tokens=[], **KW)
    _equal(again[0], _device(eng, 1, 3)[0])
    assert again[0][0].tolist() == _host_driven(eng, 1, 3)["tokens"]
    zero, _ = eng.generate_beam([p1, p1], [0, 5], 2, stop_tokens=[], **KW)                      # a sentence that asks for nothing
    assert len(zero[0][0]) == 0 and len(zero[1][0]) == 5
