"""GPU: beam search with a finished pool and beam sampling (csrc/gpt_beam_pool.hip) against the float64 restatement of its
definition (tests/gpt_beam_pool_ref.py, itself held against transformers on the CPU): the unit entry on rows of logits, then the
decode loop — the device loop against the reference loop driven over the engine's own single-sentence step, every hypothesis
and every pool entry with a private copy of its history — and its invariances.

Scores hold to |d| <= 1e-5 + 2^-22 |score| (the existing beam test's bound); everything discrete is compared wherever the
reference's margin is at least 1e-4, and the cases under it are counted."""
from types import SimpleNamespace as Raw

import numpy as np
import pytest

import gpt_beam_pool_ref as R
import gpt_beam_ref as RB
from mi355tts import weights as W
from mi355tts import _lib
from mi355tts.config import IndexGPTConfig
from mi355tts.indextts import IndexGPT, Sampling, beam_pool_select

pytestmark = pytest.mark.gpu
SEED = 9527
N_NEW = 16
KW = dict(repeat_value=0.7, penalty_range=3)


# ---------------------------------------------------------------------------------------------------------------
# 1: mi_gpt_beam_pool_select
# ---------------------------------------------------------------------------------------------------------------
def _device_select(kw):
    sp = kw["sampling"]
    return beam_pool_select(kw["logits"], kw["scores"], beams=kw["beams"], n=kw["n"], max_new=kw["max_new"], stop_tokens=kw["stops"],
                            pool_scores=kw["pool_score"], pool_finished=kw["pool_fin"], open=kw["open_"],
                            length_penalty=kw["length_penalty"], early_stopping=kw["early_stopping"],
                            sampling=Sampling(**sp) if isinstance(sp, dict) else sp, pen=kw["pen"])


def _check_select(kw, what, ties=False):
    """device against reference; False (nothing asserted) where the reference's margin is below R.MARGIN and `ties` is off"""
    ref = R.select(**kw)
    dev = _device_select(kw)
    if not ties and ref["margin"] < R.MARGIN:
        return False
    assert dev["cand"].tolist() == ref["cand"].tolist(), what
    assert dev["cand_stop"].tolist() == ref["cand_stop"].tolist(), what
    d = np.abs(dev["cand_acc"].astype(np.float64) - ref["cand_acc"])
    assert (d <= R.tol(ref["cand_acc"])).all(), (what, float(d.max()))
    k = len(ref["run"])
    assert dev["parents"][:k].tolist() == ref["parents"].tolist() and dev["tokens"][:k].tolist() == ref["tokens"].tolist(), what
    assert (dev["parents"][k:] == -1).all() and (dev["tokens"][k:] == -1).all(), what
    assert (np.abs(dev["scores"][:k].astype(np.float64) - ref["scores"]) <= R.tol(ref["scores"])).all(), what
    assert dev["pool_finished"].tolist() == ref["pool_fin"].tolist(), what
    assert dev["pool_src"].tolist() == [(-1 - j) if kind == "old" else j for kind, j in ref["pool_src"]], what
    assert (np.abs(dev["pool_scores"].astype(np.float64) - ref["pool_score"]) <= R.tol(ref["pool_score"])).all(), what
    assert dev["open"] == ref["open"] and dev["done"] == ref["done"], what
    return True


def _unit_cases(codes):
    for beams in R.UNIT_BEAMS:
        for n_stop in R.UNIT_NSTOP:
            K = (n_stop + 1) * beams
            if K > 64 or (codes != "K" and K > codes):
                continue
            for first in (True, False):
                for sampled in (False, True):
                    yield beams, n_stop, first, sampled


@pytest.mark.parametrize("codes", R.unit_codes())
def test_pool_select_vs_reference(codes):
    n = low = 0
    for case in _unit_cases(codes):
        n += 1
        low += not _check_select(R.unit_case(codes, *case), (codes,) + case)
    print(f"pool select, codes {codes}: {n} cases, {low} under the margin")
    assert n >= 40 and low * 20 <= n        # over all code counts: 3 of 296 (tests/test_gpt_beam_pool_ref.py holds the 5 % cap)


def test_pool_select_ties():
    """rows in steps of 0.25, identical rows and equal previous scores: exact ties inside and across rows go to the lower flat
    index, among the candidates, the running hypotheses and the new pool entries"""
    for beams in R.UNIT_BEAMS:
        for n_stop in (0, 1, 3):
            for first in (True, False):
                assert _check_select(R.tie_case(beams, n_stop, first), (beams, n_stop, first), ties=True)


def test_pool_select_sampled_ties():
    """sampling mode on the same rows with a top_p that leaves fewer than K codes: the K best of a row stay, equal values across
    the K-th place going to the lower code.  At selection 0 the K candidates ARE the kept set; later they are drawn from it.
    The draw's order is compared where the reference's margin allows."""
    across = 0
    for beams in R.UNIT_BEAMS:
        for n_stop in (0, 1, 3):
            for first in (True, False):
                kw = R.tie_case_sampled(beams, n_stop, first)
                ref = R.select(**kw)
                dev = _device_select(kw)
                kept = set(np.flatnonzero(ref["kept"]).tolist())
                got = dev["cand"].tolist()
                assert len(set(got)) == len(got) and set(got) <= kept, (beams, n_stop, first)
                if first:
                    assert set(got) == kept, (beams, n_stop, first)
                across += R.ties_across_kth(kw)
                _check_select(kw, (beams, n_stop, first, "sampled ties"))
    assert across >= 15


def test_pool_keeps_an_old_entry_over_an_equal_new_one():
    lg = np.zeros((2, 8), np.float32)
    lg[:, 3] = 5.0                                              # both rows finish with code 3 at the same acc
    kw = dict(logits=lg, pen=None, scores=np.array([-1.0, -1.0], np.float32), n=2, max_new=9, stops=[3], beams=2,
              pool_score=np.full(2, R.NEG, np.float32), pool_fin=np.zeros(2, bool), open_=True, length_penalty=0.0,
              early_stopping=False, sampling=None)
    first = _device_select(kw)
    assert first["pool_src"].tolist() == [0, 1] and first["pool_finished"].all()
    assert _check_select(kw, "first", ties=True)
    kw.update(n=3, pool_score=first["pool_scores"], pool_fin=first["pool_finished"])
    # the same two fp32 scores arrive again, bit for bit: the old entries stay.  (No reference here: it would compare its own
    # float64 scores of the new entries with the device's rounded ones of the old, which is no tie.)
    again = _device_select(kw)
    assert again["pool_src"].tolist() == [-1, -2] and not again["open"] and again["done"]
    np.testing.assert_array_equal(again["pool_scores"], first["pool_scores"])


def test_pool_select_limits():
    ok = dict(logits=np.zeros((2, 8), np.float32), pen=None, scores=np.zeros(2, np.float32), n=1, max_new=4, stops=[3], beams=2,
              pool_score=np.full(2, R.NEG, np.float32), pool_fin=np.zeros(2, bool), open_=True, length_penalty=0.0,
              early_stopping=False, sampling=None)
    bad = [dict(stops=[1, 2, 3, 4, 5, 6, 7]),                                  # 7 stop ids
           dict(stops=[1, 2, 3, 4]),                                           # K = 10 > 8 codes
           dict(length_penalty=float("nan")), dict(length_penalty=float("inf")),
           dict(n=4), dict(n=-1),
           dict(sampling=Raw(temperature=0.0, top_k=0, top_p=1.0, seed=1)),    # records the Sampling class would refuse itself
           dict(sampling=Raw(temperature=1.0, top_k=0, top_p=1.5, seed=1)),
           dict(sampling=Raw(temperature=1.0, top_k=-1, top_p=1.0, seed=1)),
           dict(sampling=Raw(temperature=1.0, top_k=3, top_p=1.0, seed=1))]    # top_k below K = 4
    for b in bad:
        with pytest.raises(_lib.MiError):
            _device_select({**ok, **b})
    with pytest.raises(_lib.MiError):
        _device_select({**ok, "logits": np.zeros((2, 16385), np.float32)})
    L = _lib.load()
    assert L.mi_gpt_beam_pool_select(None, *([None] * 2), 2, 8, 0, 4, None, 0, *([None] * 3), 0.0, 2, *([None] * 12), _lib.MI_HOST) != 0
    assert _check_select(ok, "still usable", ties=True)
    big = R.unit_case(16384, 8, 6, False, True)                 # the largest selection there is: 8 rows, 16384 codes, K = 56
    _check_select(big, "16384 x 8 x 56")


# ---------------------------------------------------------------------------------------------------------------
# 2: the decode loop
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
    e = _engine(small, 16)
    yield e
    e.close()


def _prompt(e, seed, n_text=6, n_cond=4):
    cfg = e.cfg
    conds = W.synth_normal(seed, "conds", (1, n_cond, cfg.hidden), std=0.5)
    text = (np.arange(n_text, dtype=np.int32) * 5 + seed) % (cfg.text_tokens - 2) + 2
    mh, _ = e.mel_embed(cfg.start_mel_token, 0)
    p, _ = e.concat(conds, e.text_embed(text), mh)
    return p


_GREEDY = {}


def _stops(e, seed):
    """stop ids a search is sure to meet: tokens 4 and 9 of the sentence's greedy decode"""
    if (id(e), seed) not in _GREEDY:
        res, _ = e.generate_batch([_prompt(e, seed)], [N_NEW], stop_tokens=[], **KW)
        _GREEDY[id(e), seed] = res[0][0].tolist()
    g = _GREEDY[id(e), seed]
    return tuple(dict.fromkeys((g[4], g[9])))


def _sp(seed):
    return Sampling(1.0, 30, 0.8, 1000 + seed)


def _device(e, seed, beams, lp, es, sampled, stops=None, max_new=N_NEW):
    res, _ = e.generate_beam([_prompt(e, seed)], [max_new], beams, stop_tokens=list(_stops(e, seed) if stops is None else stops),
                             pool=True, length_penalty=lp, early_stopping=es, sampling=_sp(seed) if sampled else None, **KW)
    return res[0]


_HOST = {}


def _host_driven(e, seed, beams, lp, es, sampled):
    key = (seed, beams, lp, es, sampled)
    if key not in _HOST:
        sp = _sp(seed)
        _HOST[key] = R.pool_generate(RB.EngineModel(e), _prompt(e, seed), beams, N_NEW, stop_tokens=_stops(e, seed),
                                     length_penalty=lp, early_stopping=es,
                                     sampling=dict(temperature=sp.temperature, top_k=sp.top_k, top_p=sp.top_p, seed=sp.seed)
                                     if sampled else None, **KW)
    return _HOST[key]


# beams 2-5 x (length_penalty, early_stopping) x both modes, the seeds going round 1-3
CASES = [(1 + (b + q) % 3, b, lp, es, sampled) for sampled in (False, True) for b in (2, 3, 4, 5)
         for q, (lp, es) in enumerate(((0.0, False), (1.0, False), (0.0, True), (1.0, True)))]


def _compare(dev, ref, what):
    toks, hid, score = dev
    d = abs(score - ref["score"])
    print(f"pool {what}: min margin {min(ref['margins']):.3g}, {len(toks)} tokens, score {score:.6f} (host-driven {ref['score']:.6f}, "
          f"|d| {d:.3g}), pool-decided {ref['from_pool_only']}, ended by open {ref['ended_by_open']}")
    assert toks.tolist() == ref["tokens"], what
    assert d <= R.tol(ref["score"]), what
    assert hid.shape == ref["hidden"].shape
    np.testing.assert_allclose(hid, ref["hidden"], rtol=0, atol=2e-4)


@pytest.mark.parametrize("seed,beams,lp,es,sampled", CASES)
def test_device_pool_vs_host_driven(eng, seed, beams, lp, es, sampled):
    ref = _host_driven(eng, seed, beams, lp, es, sampled)
    dev = _device(eng, seed, beams, lp, es, sampled)
    if min(ref["margins"]) < R.MARGIN:                                # counted by test_enough_pool_cases_are_compared
        print(f"pool {(seed, beams, lp, es, sampled)}: host-side margin {min(ref['margins']):.3g} below {R.MARGIN}, not compared")
        return
    _compare(dev, ref, (seed, beams, lp, es, sampled))


def test_enough_pool_cases_are_compared(eng):
    refs = [(c, _host_driven(eng, *c)) for c in CASES]
    full = [(c, r) for c, r in refs if min(r["margins"]) >= R.MARGIN]
    assert len(CASES) == 32 and 2 * len(full) >= len(CASES), len(full)
    for sampled in (False, True):                                     # per mode: an answer only the pool could give
        assert any(r["from_pool_only"] for c, r in full if c[4] == sampled), sampled
    assert any(r["ended_by_open"] for c, r in full)                   # and a search that `open` ended before any limit


def _equal(a, b):
    assert a[0].tolist() == b[0].tolist() and a[2] == b[2]           # tokens and score, bit for bit
    np.testing.assert_array_equal(a[1], b[1])


def test_one_pool_beam_is_greedy(eng):
    for seed in (1, 2):
        p = _prompt(eng, seed)
        for stops in ([], list(_stops(eng, seed))):
            rb, _ = eng.generate_batch([p], [N_NEW], stop_tokens=stops, **KW)
            t1, h1, _ = _device(eng, seed, 1, 0.0, False, False, stops=stops)
            assert t1.tolist() == rb[0][0].tolist(), (seed, stops)
            np.testing.assert_allclose(h1, rb[0][1], rtol=0, atol=2e-4)


def test_pool_groups_do_not_see_each_other(eng):
    seeds, lim = (1, 2, 3), [N_NEW, 11, 14]
    ps = [_prompt(eng, s, n_text=6 + s) for s in seeds]
    sps = [_sp(s) for s in seeds]
    for sampling in (None, sps):
        for stops in ([], list(_stops(eng, 1))):
            kw = dict(stop_tokens=stops, pool=True, length_penalty=1.0, **KW)
            three, _ = eng.generate_beam(ps, lim, 3, sampling=sampling, **kw)
            for g in range(3):
                alone, _ = eng.generate_beam([ps[g]], [lim[g]], 3, sampling=None if sampling is None else sps[g], **kw)
                _equal(three[g], alone[0])
    # a sampled sentence does not depend on its slot or on nb
    twice, _ = eng.generate_beam([ps[0], ps[1], ps[0]], [N_NEW] * 3, 3, sampling=[sps[0], sps[1], sps[0]], stop_tokens=[], pool=True, **KW)
    _equal(twice[0], twice[2])


def test_pool_graph_replay_equals_eager(eng):
    ps = [_prompt(eng, 3), _prompt(eng, 1)]
    for sampling in (None, [_sp(3), _sp(1)]):
        kw = dict(stop_tokens=list(_stops(eng, 3)), pool=True, sampling=sampling, **KW)
        a, _ = eng.generate_beam(ps, [N_NEW, N_NEW], 3, **kw)
        a2, _ = eng.generate_beam(ps, [N_NEW, N_NEW], 3, **kw)           # the captured graph by now
        _lib.prof_reset(); _lib.prof_enable(("attn",))                    # profiling: eager launches
        try:
            b, _ = eng.generate_beam(ps, [N_NEW, N_NEW], 3, **kw)
        finally:
            _lib.prof_enable(())
        for g in range(2):
            _equal(a[g], b[g])
            _equal(a[g], a2[g])


def _lead(margins, bound):
    k = 0
    while k < len(margins) and margins[k] >= bound:
        k += 1
    return k


@pytest.mark.parametrize("dtype,eps", [("f16", 2.0 ** -11), ("bf16", 2.0 ** -8)])
def test_pool_16_bit_engines(small, dtype, eps):
    """The 16-bit engines against their own host-driven loop.  That loop reads its logits from the single-sentence step, the device
    loop from the batched one: two kernels that round the same 16-bit activations in different places, so a logit may differ by
    one 16-bit rounding of a logit-sized quantity, d = eps * zmax (eps = half an ulp of the format, zmax = the largest
    |logits * pen| the host-driven loop read), and a log-probability z - lse(z) by 2 d.  A selection is decided when its host-side
    margin is at least 4 d (a gap between two candidates that 2 d on each cannot close).  Few 16-selection runs are decided
    throughout, so per mode the case is searched here, on the host-driven loop alone: over seeds 1-6, 3 and 2 beams and two, one
    and no stop id, the run with the most decided leading selections, cut to that many tokens (max_new: the last selection
    then finishes every candidate, so the pool and the gather are in it) and cut further until every selection of the cut run is
    decided.  That case must exist, and the device must give its tokens and rows, and its score to len(tokens) * 2 d.  One beam
    against generate_batch, which reads the same batched step, is compared exactly."""
    e = _engine(small, 3, dtype)

    def host(seed, beams, stops, sampled, max_new):
        sp = _sp(seed)
        return R.pool_generate(RB.EngineModel(e), _prompt(e, seed), beams, max_new, stop_tokens=stops, length_penalty=0.0,
                               sampling=dict(temperature=sp.temperature, top_k=sp.top_k, top_p=sp.top_p, seed=sp.seed)
                               if sampled else None, **KW)

    for sampled in (False, True):
        best = None
        for seed in range(1, 7):
            both = _stops(e, seed)
            for beams in (3, 2):
                for stops in (both, both[:1], ()):
                    ref = host(seed, beams, stops, sampled, N_NEW)
                    k = _lead(ref["margins"], 4 * eps * ref["zmax"])
                    if best is None or k > best[0]:
                        best = (k, seed, beams, stops, len(ref["margins"]))
        k, seed, beams, stops, n_sel = best
        m = N_NEW if k == n_sel else k
        ref = None
        while m >= 1:
            ref = host(seed, beams, stops, sampled, m)
            d = eps * ref["zmax"]
            if min(ref["margins"]) >= 4 * d:
                break
            m, ref = m - 1, None
        assert ref is not None, (dtype, sampled, best)                # a case decided throughout exists
        toks, hid, score = _device(e, seed, beams, 0.0, False, sampled, stops=stops, max_new=m)
        print(f"pool {dtype} sampled={sampled}: seed {seed}, {beams} beams, {len(stops)} stop ids, max_new {m}: {len(toks)} tokens, "
              f"min margin {min(ref['margins']):.3g}, 4 d = {4 * d:.3g}, score {score:.6f} / {ref['score']:.6f}")
        assert toks.tolist() == ref["tokens"], (dtype, sampled)
        assert abs(score - ref["score"]) <= len(toks) * 2 * d + R.tol(ref["score"]), (dtype, sampled)
        assert hid.shape == ref["hidden"].shape and np.isfinite(hid).all()
    p = _prompt(e, 2)
    gb, _ = e.generate_batch([p], [N_NEW], stop_tokens=[], **KW)
    one, _ = e.generate_beam([p], [N_NEW], 1, stop_tokens=[], pool=True, **KW)
    assert one[0][0].tolist() == gb[0][0].tolist()
    for seed in range(1, 7):
        _GREEDY.pop((id(e), seed), None)
    e.close()


def test_greedy_sampled_beam_pool_on_one_handle(eng, small):
    """greedy, sampled, old beam and the two pool calls interleaved on one handle, twice over, give what each gives as the first
    call on a fresh handle"""
    p = _prompt(eng, 1)
    ones = np.ones((1, eng.cfg.mel_codes), np.float32)
    sp = Sampling(1.0, 30, 0.8, 31)
    calls = [lambda e: e.generate_from_prompt(p, N_NEW, stop_tokens=[], repeat_penality=ones, **KW),
             lambda e: e.generate_from_prompt(p, N_NEW, stop_tokens=[], repeat_penality=ones, sampling=sp, **KW),
             lambda e: e.generate_beam([p], [N_NEW], 3, stop_tokens=[], **KW)[0][0],
             lambda e: _device(e, 1, 3, 0.0, False, False, stops=stops),
             lambda e: _device(e, 1, 3, 0.0, False, True, stops=stops)]
    stops = _stops(eng, 1)
    fresh = []
    for c in calls:
        e = _engine(small, 16)
        fresh.append(c(e))
        e.close()
    for _ in range(2):
        got = [c(eng) for c in calls]
        for a, b in zip(fresh[:2], got[:2]):                     # (tokens, rows, penalty)
            assert a[0].tolist() == b[0].tolist()
            np.testing.assert_array_equal(a[1], b[1])
        for a, b in zip(fresh[2:], got[2:]):                     # (tokens, rows, score)
            _equal(a, b)


def test_pool_limits(eng):
    cfg = eng.cfg
    p1 = np.ascontiguousarray(_prompt(eng, 1), dtype=np.float32)
    with pytest.raises(ValueError):
        eng.generate_beam([p1], [4], 3, stop_tokens=[], sampling=_sp(1))                        # sampling needs pool=True
    L = _lib.load()
    n = np.zeros(1, np.int32)
    toks = np.zeros((1, 4), np.int32)
    rows = np.array([p1.shape[1]], np.int32)
    mx = np.array([4], np.int32)
    stops = np.arange(6, dtype=np.int32)
    T, K, P, S = np.array([1.0], np.float32), np.array([30], np.int32), np.array([0.8], np.float32), np.array([5], np.uint64)

    def call(nb=1, beams=3, n_stop=1, lp=0.0, es=0, samp=(None,) * 4):
        return L.mi_gpt_generate_beam_pool(eng._h, nb, p1.ctypes.data, _lib.i32p(rows), _lib.i32p(mx), stops.ctypes.data, n_stop, 0.7, 3,
                                           None, beams, lp, es, *samp, toks.ctypes.data, None, 4, _lib.i32p(n), None, _lib.MI_HOST)

    sa = (T.ctypes.data, K.ctypes.data, P.ctypes.data, S.ctypes.data)
    assert call() == 0 and call(samp=sa) == 0
    K8 = np.array([8], np.int32)
    bad = [dict(beams=0), dict(beams=9), dict(beams=8, n_stop=6),                               # K = 56 > 50 mel codes
           dict(lp=float("nan")), dict(lp=float("-inf")), dict(es=2), dict(es=-1),
           dict(samp=(T.ctypes.data, None, None, None)),                                        # only some of the four arrays
           dict(samp=(np.array([0.0], np.float32).ctypes.data,) + sa[1:]),
           dict(samp=(sa[0], sa[1], np.array([0.0], np.float32).ctypes.data, sa[3])),
           dict(beams=3, n_stop=3, samp=(sa[0], K8.ctypes.data, sa[2], sa[3]))]                 # top_k = 8 below K = 12
    for b in bad:
        assert call(**b) != 0, b
    assert cfg.mel_codes < 64 and call(beams=8, n_stop=5) == 0                                  # K = 48 fits
    a = _device(eng, 1, 3, 0.0, False, False)                                                    # the handle still decodes
    _equal(a, _device(eng, 1, 3, 0.0, False, False))
    res, _ = eng.generate_beam([p1, p1], [0, 5], 2, stop_tokens=[], pool=True, **KW)             # a sentence that asks for nothing
    assert len(res[0][0]) == 0 and len(res[1][0]) == 5 and res[0][2] == 0.0 and res[1][2] < 0.0
