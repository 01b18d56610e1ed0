"""GPU: seeded temperature / top-k / top-p sampling of the IndexTTS GPT (csrc/gpt_sample.hip) against the float64 restatement of
its definition (tests/gpt_sampling_ref.py): the unit entry on rows of logits, then the decode loop end to end and its
invariances (seed, slot, batch, graph replay, mode switches on one handle).

z and u are exactly reproducible on the host, so set membership and u are compared bit for bit; probabilities within 1e-5;
tokens wherever the reference's margin says rounding cannot decide."""
import types

import numpy as np
import pytest

import gpt_sampling_ref as R
from mi355tts import weights as W
from mi355tts import _lib
from mi355tts.config import IndexGPTConfig
from mi355tts.indextts import IndexGPT, Sampling, sample_logits
from oracle import gpt_np as O

pytestmark = pytest.mark.gpu
SEED = 9527
EPS = 1e-5


# ---------------------------------------------------------------------------------------------------------------
# 1-3: mi_gpt_sample_logits
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 3, 16])
@pytest.mark.parametrize("codes", R.CODES)
def test_sample_logits_vs_reference(codes, rows):
    c = R.cases(codes)
    lg, pen = c["logits"][:rows], c["pen"][:rows]
    n_cases = borderline = 0
    for (k, p, t), (seeds, pos, refs) in c["refs"].items():
        toks, u, probs = sample_logits(lg, pen=pen, temperature=t, top_k=k, top_p=p, seeds=seeds[:rows], positions=pos[:rows],
                                       return_probs=True)
        for r in range(rows):
            ref = refs[r]
            assert u[r] == ref["u"], (k, p, t, r)                                        # bit-equal draw
            if p == 1.0:
                np.testing.assert_array_equal(probs[r] > 0, ref["K"], err_msg=str((k, p, t, r)))   # K: pure fp32 comparison
            assert np.abs(probs[r].astype(np.float64) - ref["probs"]).max() <= 1e-5, (k, p, t, r)
            n_cases += 1
            if ref["margin"] < EPS:
                borderline += 1
            else:
                assert toks[r] == ref["token"], (k, p, t, r, float(ref["margin"]))
    assert n_cases == 72 * rows and borderline <= n_cases // 100


def test_sample_logits_tie_row():
    """logits in steps of 0.25 at temperature 1: exact ties straddle t_k and t_p; the kept set is the reference's, tie-closed"""
    tr = R.tie_row()
    for k, p in ((30, 0.8), (30, 1.0), (0, 0.5), (0, 1.0), (2, 0.8)):
        ref = R.sample(tr, None, 1.0, k, p, 5, 3)
        assert ref["margin"] > 1e-4
        toks, u, probs = sample_logits(tr[None], temperature=1.0, top_k=k, top_p=p, seeds=5, positions=3, return_probs=True)
        np.testing.assert_array_equal(probs[0] > 0, ref["P"], err_msg=str((k, p)))
        assert np.abs(probs[0].astype(np.float64) - ref["probs"]).max() <= 1e-5
        assert u[0] == ref["u"] and toks[0] == ref["token"]


def test_sample_logits_frequencies():
    lg = R.freq_row()
    ref = R.sample(lg, None, 1.0, 30, 0.8, R.FREQ_SEED, 0)
    toks, u = sample_logits(np.tile(lg, (R.FREQ_N, 1)), temperature=1.0, top_k=30, top_p=0.8, seeds=R.FREQ_SEED,
                            positions=np.arange(R.FREQ_N))
    assert ref["P"][toks].all()                                   # only codes of the reference's P occur
    assert R.freq_ok(toks, ref)
    for n in (0, 1, 1000, R.FREQ_N - 1):
        assert u[n] == R.uniform(R.FREQ_SEED, n)


def test_sample_logits_errors_and_code_range():
    lg = np.zeros((1, 8), np.float32)
    ok = dict(temperature=1.0, top_k=3, top_p=0.9, seeds=1, positions=0)
    for bad in (dict(temperature=0.0), dict(temperature=-2.0), dict(temperature=np.nan), dict(temperature=np.inf),
                dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=np.nan), dict(positions=-1)):
        with pytest.raises(_lib.MiError):
            sample_logits(lg, **{**ok, **bad})
    with pytest.raises(_lib.MiError):
        sample_logits(np.zeros((1, 16385), np.float32), **ok)     # above the register tile: an error, not a wrong answer
    # 1 code and the largest supported count
    toks, _ = sample_logits(np.zeros((1, 1), np.float32), **ok)
    assert toks[0] == 0
    rng = np.random.default_rng(4)
    big = (rng.standard_normal(16384) * 3).astype(np.float32)
    toks, u, probs = sample_logits(big[None], temperature=1.0, top_k=50, top_p=0.9, seeds=3, positions=7, return_probs=True)
    ref = R.sample(big, None, 1.0, 50, 0.9, 3, 7)
    np.testing.assert_array_equal(probs[0] > 0, ref["P"])
    assert ref["margin"] < EPS or toks[0] == ref["token"]


# ---------------------------------------------------------------------------------------------------------------
# 4-7: the decode loop
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    cfg = IndexGPTConfig.small()
    return cfg, W.synth_state(W.gpt_spec(cfg), SEED)


@pytest.fixture(scope="module")
def eng(small):
    cfg, st = small
    e = IndexGPT(cfg, st, dtype="f32")
    yield e
    e.close()


@pytest.fixture(scope="module")
def beng(small):
    cfg0, st = small
    cfg = IndexGPTConfig(**{**cfg0.__dict__, "max_batch": 4})
    e = IndexGPT(cfg, st, dtype="f32")
    yield e
    e.close()


def _prompt(e, cfg, seed, n_text, n_cond=4):
    conds = W.synth_normal(seed, "conds", (1, n_cond, cfg.hidden), std=0.5)
    text = (np.arange(n_text, dtype=np.int32) * 5 + seed) % (cfg.text_tokens - 2) + 2
    mh, _ = e.mel_embed(cfg.start_mel_token, 0)
    p, _ = e.concat(conds, e.text_embed(text), mh)
    return p


def _ones(cfg, nb=1):
    return np.ones((nb, cfg.mel_codes), np.float32)


def _single(e, p, limit, sampling, stop_tokens=()):
    return e.generate_from_prompt(p, limit, stop_tokens=list(stop_tokens), repeat_penality=_ones(e.cfg), sampling=sampling)


def test_top_k_1_is_greedy(eng, beng):
    cfg = eng.cfg
    p = _prompt(eng, cfg, 1, 6)
    t0, h0, p0 = _single(eng, p, 20, None)
    t1, h1, p1 = _single(eng, p, 20, Sampling(top_k=1, temperature=0.6, top_p=0.3, seed=5))
    assert len(t0) == 20 and t1.tolist() == t0.tolist()
    np.testing.assert_array_equal(h1, h0)
    np.testing.assert_array_equal(p1, p0)
    ps = [_prompt(beng, cfg, s, n) for s, n in ((1, 6), (2, 3), (3, 9))]
    lim = [12, 9, 14]
    r0, pen0 = beng.generate_batch(ps, lim, stop_tokens=[])
    r1, pen1 = beng.generate_batch(ps, lim, stop_tokens=[], sampling=[Sampling(top_k=1, seed=b) for b in range(3)])
    for b in range(3):
        assert r1[b][0].tolist() == r0[b][0].tolist() and len(r0[b][0]) == lim[b]
        np.testing.assert_array_equal(r1[b][1], r0[b][1])
    np.testing.assert_array_equal(pen1, pen0)


def _teacher_forced_hidden(cfg, st, prompt, toks):
    """Oracle hidden states and logits when it is fed the ENGINE's tokens"""
    keys = [np.zeros((cfg.heads, 64, 0), np.float32)] * cfg.layers
    vals = [np.zeros((cfg.heads, 0, 64), np.float32)] * cfg.layers
    pen = np.ones((1, cfg.mel_codes), np.float32)
    folds = [O.fold_layer(cfg, st, i) for i in range(cfg.layers)]
    keys, vals, kvl, last, _, logits = O.graph_e(cfg, st, keys, vals, 0, pen, prompt.shape[1], prompt, 1, folds)
    out, lg = [last], [logits]
    gl = np.array([1])
    for t in toks[:-1]:
        hs, gl = O.graph_c(cfg, st, [[int(t)]], gl)
        keys, vals, kvl, last, _, logits = O.graph_e(cfg, st, keys, vals, int(kvl[0]), pen, 1, hs, 0, folds)
        out.append(last); lg.append(logits)
    return np.concatenate(out, 0), np.concatenate(lg, 0)


def test_sampled_decode_vs_oracle(eng, small):
    """40 sampled tokens of the small fp32 model; at every step the reference sampler, run on the ORACLE's logits for the engine's
    own token history, picks the engine's token unless the step is borderline.  eps = 10 x the largest |engine logits - oracle
    logits| of the run relative to the logit spread (measured here, not chosen, and printed).
    First run on an MI355X: max |engine - oracle logits| 1.01e-6 over a spread of 7.4 -> eps 1.37e-6; no step borderline."""
    cfg, st = small
    sp = Sampling(1.0, 30, 0.8, 1234)
    p = _prompt(eng, cfg, 1, 6)
    n_new = 40
    toks, hid, pen = _single(eng, p, n_new, sp)
    assert len(toks) == n_new
    ohid, ologits = _teacher_forced_hidden(cfg, st, p, toks)
    np.testing.assert_allclose(hid, ohid, rtol=0, atol=3e-4)
    # the engine's own logits along the same history (the kernels of the decode step, one mi_gpt_step per token)
    eng.reset()
    hs, gl, flag, elog = p, np.array([1]), 1, []
    for n, t in enumerate(toks):
        _, _, _, lg = eng.step(hs, _ones(cfg), attention_mask=flag, return_logits=True)
        elog.append(lg[0])
        if n + 1 < n_new:
            hs, gl = eng.mel_embed(int(t), gl)
        flag = 0
    elog = np.stack(elog)
    dmax = float(np.abs(elog - ologits).max())
    spread = float(ologits.max() - ologits.min())
    eps = 10.0 * dmax / spread
    before, pen_end = R.bookkeeping(toks, cfg.mel_codes, cfg.repeat_penalty, cfg.penalty_range, [])
    borderline = 0
    for n in range(n_new):
        ref = R.sample(ologits[n], before[n], sp.temperature, sp.top_k, sp.top_p, sp.seed, n)
        if ref["margin"] < eps:
            borderline += 1
        else:
            assert int(toks[n]) == ref["token"], (n, float(ref["margin"]), eps)
    print(f"sampled decode: max |dlogits| {dmax:.3g}, spread {spread:.3g}, eps {eps:.3g}, borderline {borderline}")
    assert borderline <= 1
    np.testing.assert_array_equal(pen[0], pen_end)
    assert len(set(toks.tolist())) > 3                           # it does sample


def test_seed_decides_the_take(eng):
    cfg = eng.cfg
    p = _prompt(eng, cfg, 2, 5)
    a = _single(eng, p, 40, Sampling(1.0, 30, 0.8, 7))
    b = _single(eng, p, 40, Sampling(1.0, 30, 0.8, 7))
    c = _single(eng, p, 40, Sampling(1.0, 30, 0.8, 8))
    d = _single(eng, p, 40, Sampling(1.0, 30, 0.8, 7 + (1 << 32)))          # the high seed word is part of the key
    assert len(a[0]) == 40 and a[0].tolist() == b[0].tolist()
    np.testing.assert_array_equal(a[1], b[1])
    assert a[0].tolist() != c[0].tolist() and a[0].tolist() != d[0].tolist()


def test_batch_equals_single_and_slots_permute(beng):
    cfg = beng.cfg
    ps = [_prompt(beng, cfg, s, n) for s, n in ((1, 6), (2, 3), (3, 9))]
    lim = [22, 9, 17]
    sp = [Sampling(1.0, 30, 0.8, 11), None, Sampling(1.4, 0, 0.95, 12)]
    res, pen = beng.generate_batch(ps, lim, stop_tokens=[], sampling=sp)
    for b in range(3):
        t, h, pn = _single(beng, ps[b], lim[b], sp[b])
        assert len(t) == lim[b] and res[b][0].tolist() == t.tolist(), b
        # tokens and penalties bit-equal; the last_hidden_state rows of the two paths leave different LayerNorm kernels (fused
        # into the GEMV / on its own), the bar test_gpu_gpt.py holds the greedy paths to
        np.testing.assert_allclose(res[b][1], h, rtol=0, atol=2e-4)
        np.testing.assert_array_equal(pen[b:b + 1], pn)
    assert res[0][0].tolist() != _single(beng, ps[0], lim[0], None)[0].tolist()
    perm = [2, 0, 1]
    res2, pen2 = beng.generate_batch([ps[i] for i in perm], [lim[i] for i in perm], stop_tokens=[], sampling=[sp[i] for i in perm])
    for slot, i in enumerate(perm):
        assert res2[slot][0].tolist() == res[i][0].tolist()
        np.testing.assert_array_equal(res2[slot][1], res[i][1])
        np.testing.assert_array_equal(pen2[slot], pen[i])
    # one Sampling for every sentence: the same seed and prompt in two slots give the same take
    res3, _ = beng.generate_batch([ps[0], ps[0]], [15, 15], stop_tokens=[], sampling=Sampling(1.0, 30, 0.8, 11))
    assert res3[0][0].tolist() == res3[1][0].tolist() == res[0][0][:15].tolist()
    with pytest.raises(ValueError):
        beng.generate_batch(ps, lim, sampling=[Sampling()])


def test_graph_replay_equals_eager_sampled(small, monkeypatch):
    cfg0, st = small
    cfg = IndexGPTConfig(**{**cfg0.__dict__, "max_batch": 2})
    a = IndexGPT(cfg, st, dtype="f16")
    monkeypatch.setenv("MI355TTS_NO_GRAPH", "1")
    b = IndexGPT(cfg, st, dtype="f16")
    monkeypatch.delenv("MI355TTS_NO_GRAPH")
    p, p2 = _prompt(a, cfg, 1, 6), _prompt(a, cfg, 2, 4)
    sp = Sampling(1.0, 30, 0.8, 21)
    for _ in range(2):
        ta, ha, _ = _single(a, p, 20, sp)
        tb, hb, _ = _single(b, p, 20, sp)
        assert ta.tolist() == tb.tolist() and len(ta) == 20
        np.testing.assert_array_equal(ha, hb)
        ra, _ = a.generate_batch([p, p2], [20, 18], stop_tokens=[], sampling=[sp, Sampling(0.8, 10, 1.0, 22)])
        rb, _ = b.generate_batch([p, p2], [20, 18], stop_tokens=[], sampling=[sp, Sampling(0.8, 10, 1.0, 22)])
        for s in range(2):
            assert ra[s][0].tolist() == rb[s][0].tolist()
            np.testing.assert_array_equal(ra[s][1], rb[s][1])
    a.close()
    b.close()


def test_greedy_sampled_greedy_on_one_handle(beng):
    cfg = beng.cfg
    p, p2 = _prompt(beng, cfg, 1, 6), _prompt(beng, cfg, 2, 4)
    sp = Sampling(1.0, 30, 0.8, 31)
    g0 = _single(beng, p, 40, None)
    s0 = _single(beng, p, 40, sp)
    g1 = _single(beng, p, 40, None)
    s1 = _single(beng, p, 40, sp)
    assert g0[0].tolist() == g1[0].tolist() and s0[0].tolist() == s1[0].tolist() and g0[0].tolist() != s0[0].tolist()
    np.testing.assert_array_equal(g0[1], g1[1])
    np.testing.assert_array_equal(s0[1], s1[1])
    b0, _ = beng.generate_batch([p, p2], [40, 30], stop_tokens=[])
    bs, _ = beng.generate_batch([p, p2], [40, 30], stop_tokens=[], sampling=sp)
    b1, _ = beng.generate_batch([p, p2], [40, 30], stop_tokens=[])
    for s in range(2):
        assert b0[s][0].tolist() == b1[s][0].tolist()
        np.testing.assert_array_equal(b0[s][1], b1[s][1])
    assert bs[0][0].tolist() == s0[0].tolist() and b0[0][0].tolist() == g0[0].tolist()
    # the drop-in step entry stays greedy after a sampled call
    beng.reset()
    _, _, tok, lg = beng.step(p, _ones(cfg), attention_mask=1, return_logits=True)
    assert int(tok[0, 0]) == int(np.argmax(lg)) == int(g0[0][0])


def test_sampled_stop_token_ends_the_sentence(eng):
    cfg = eng.cfg
    p = _prompt(eng, cfg, 3, 7)
    sp = Sampling(1.0, 30, 0.8, 41)
    free, _, _ = _single(eng, p, 30, sp)
    stop = int(free[6])
    first = free.tolist().index(stop)
    toks, hid, pen = _single(eng, p, 30, sp, stop_tokens=[stop, 1000])
    assert toks.tolist() == free[: first + 1].tolist() and hid.shape == (first + 1, cfg.hidden)
    _, pen_end = R.bookkeeping(toks, cfg.mel_codes, cfg.repeat_penalty, cfg.penalty_range, [stop, 1000])
    np.testing.assert_array_equal(pen[0], pen_end)
    assert pen_end[stop] == 1.0 or stop in toks[:first].tolist()      # the stop token itself is not penalised


def test_sampling_errors_leave_the_handle_usable(eng, beng):
    cfg = eng.cfg
    p = _prompt(eng, cfg, 1, 6)
    good = _single(eng, p, 12, Sampling(1.0, 30, 0.8, 3))
    for bad in (dict(temperature=0.0), dict(temperature=float("nan")), dict(temperature=float("inf")), dict(top_k=-1),
                dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan"))):
        raw = types.SimpleNamespace(**{**dict(temperature=1.0, top_k=30, top_p=0.8, seed=3), **bad})    # past the dataclass's checks
        with pytest.raises(_lib.MiError):
            _single(eng, p, 12, raw)
    again = _single(eng, p, 12, Sampling(1.0, 30, 0.8, 3))
    assert again[0].tolist() == good[0].tolist()
    assert len(_single(eng, p, 12, None)[0]) == 12
    # the batched entry validates every item
    L = _lib.load()
    ps = np.ascontiguousarray(np.concatenate([p[0], p[0]], 0))
    rows = np.array([p.shape[1]] * 2, np.int32); mx = np.array([4, 4], np.int32); n = np.zeros(2, np.int32)
    toks = np.zeros((2, 4), np.int32); hid = np.zeros((2, 4, cfg.hidden), np.float32)
    T = np.array([1.0, -1.0], np.float32); K = np.array([30, 30], np.int32); Pp = np.array([0.8, 0.8], np.float32)
    Sd = np.array([1, 2], np.uint64)
    rc = L.mi_gpt_generate_batch_sampled(beng._h, 2, ps.ctypes.data, _lib.i32p(rows), _lib.i32p(mx), None, 0, 0.7, 10, None,
                                         toks.ctypes.data, hid.ctypes.data, 4, _lib.i32p(n), _lib.MI_HOST, T.ctypes.data,
                                         K.ctypes.data, Pp.ctypes.data, Sd.ctypes.data)
    assert rc != 0 and b"temperature" in L.mi_last_error()
    res, _ = beng.generate_batch([p, p], [4, 4], stop_tokens=[], sampling=Sampling(1.0, 30, 0.8, 3))
    assert res[0][0].tolist() == good[0][:4].tolist()
