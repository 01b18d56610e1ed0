"""GPU: pool-mode beam search and beam sampling through the sentence queue (mi_gpt_generate_queue_beam_pool /
mi_gpt_queue_begin_beam_pool; IndexGPT.generate_queue and queue_session with ``beams`` and ``pool=True``): a sentence runs "beam
search with a finished pool" as a group of B consecutive slots, the queue schedules groups, a pass makes the pools of the groups it
admits empty and runs their selection 0 in one launch, and a finished group leaves along its pool entry 0's frozen list ahead of
the pass that refills it.

Per sentence the result has to be what mi_gpt_generate_beam_pool gives for that sentence alone from a penalty vector of ones.
Bars, all the project's own: tokens equal; |score difference| <= gpt_beam_pool_ref.tol; rows within 2e-4 of the engine's alone run;
and against the definition's loop driven on the host over the engine's own single-sentence step (gpt_beam_pool_ref.pool_generate
over gpt_beam_ref.EngineModel): tokens equal and the score within tol.  Tokens are compared where rounding cannot decide: the
host-driven margin of every one of the eight sentences has to be at least R.MARGIN = 1e-4 in every configuration, and that is
asserted: none is skipped.  The entry's stats are held against queue_schedule(..., beams=B) over the SELECTIONS each sentence
ran (one margin per selection), not over the lengths returned, which in pool mode are pool entry 0's.

The eight sentences are those of tests/test_gpu_gpt_queue_beam.py, stop id 3; sampled mode is Sampling(1.0, 30, 0.8, 1001 + i) for
sentence i.  Three modes: deterministic with length_penalty 0; sampled with length_penalty 1; deterministic with length_penalty 1
and early stopping."""
import numpy as np
import pytest

import gpt_beam_pool_ref as R
import gpt_beam_ref as RB
from mi355tts import weights as W
from mi355tts import _lib
from mi355tts.config import IndexGPTConfig
from mi355tts.indextts import IndexGPT, Sampling, queue_schedule

pytestmark = pytest.mark.gpu
SEED = 9527
KW = dict(repeat_value=0.7, penalty_range=3)
TEXT = (6, 3, 9, 5, 1, 8, 4, 7)
LIMITS = [14, 9, 11, 3, 12, 1, 10, 6]
STOPS = (3,)
MI_ESTATE = -4            # include/mi355tts.h
# name -> (length_penalty, early_stopping, sampled)
MODES = {"det": (0.0, False, False), "sampled": (1.0, False, True), "early": (1.0, True, False)}


def _sp(i):
    return Sampling(1.0, 30, 0.8, 1001 + i)


def _prompt(e, seed, n_text, n_cond=4):
    cfg = e.cfg
    conds = W.synth_normal(seed, "conds", (1, n_cond, cfg.hidden), std=0.5)
    text = (np.arange(n_text, dtype=np.int32) * 5 + seed) % (cfg.text_tokens - 2) + 2
    mh, _ = e.mel_embed(cfg.start_mel_token, 0)
    p, _ = e.concat(conds, e.text_embed(text), mh)
    return p


@pytest.fixture(scope="module")
def small():
    cfg = IndexGPTConfig.small()
    return cfg, W.synth_state(W.gpt_spec(cfg), SEED)


def _engine(small, max_batch, dtype="f32"):
    cfg0, st = small
    return IndexGPT(IndexGPTConfig(**{**cfg0.__dict__, "max_batch": max_batch}), st, dtype=dtype)


def _pool_kw(mode, sampling):
    lp, es, _ = MODES[mode]
    return dict(pool=True, length_penalty=lp, early_stopping=es, sampling=sampling)


class _Ctx:
    """an engine, the eight sentences, and every sentence's alone run (mi_gpt_generate_beam_pool, one group) and host-driven run,
    once each"""

    def __init__(self, small, max_batch, beams):
        self.e = _engine(small, max_batch)
        self.cfg, self.beams = self.e.cfg, beams
        self.prompts = [_prompt(self.e, 1 + b, TEXT[b]) for b in range(8)]
        self._alone, self._host = {}, {}

    def samplings(self, mode, idx=range(8)):
        return [_sp(i) for i in idx] if MODES[mode][2] else None

    def alone(self, i, limit, mode, stops=STOPS, sp=None):
        sp = (_sp(i) if MODES[mode][2] else None) if sp is None else sp
        key = (i, limit, mode, tuple(stops), None if sp is None else sp.seed)
        if key not in self._alone:
            res, _ = self.e.generate_beam([self.prompts[i]], [limit], self.beams, stop_tokens=list(stops), **_pool_kw(mode, sp), **KW)
            self._alone[key] = res[0]
        return self._alone[key]

    def host(self, i, mode, stops=STOPS):
        """the definition's loop over the engine's own single-sentence step (every hypothesis with its own cache copy)"""
        key = (i, mode, tuple(stops))
        if key not in self._host:
            lp, es, sampled = MODES[mode]
            sp = _sp(i)
            self._host[key] = R.pool_generate(RB.EngineModel(self.e), self.prompts[i], self.beams, LIMITS[i], stop_tokens=stops,
                                              length_penalty=lp, early_stopping=es,
                                              sampling=dict(temperature=sp.temperature, top_k=sp.top_k, top_p=sp.top_p, seed=sp.seed)
                                              if sampled else None, **KW)
        return self._host[key]

    def queue(self, idx, limits, mode, stops=STOPS, sampling="mode", **kw):
        sampling = self.samplings(mode, idx) if isinstance(sampling, str) else sampling
        return self.e.generate_queue([self.prompts[i] for i in idx], limits, stop_tokens=list(stops), beams=self.beams,
                                     return_stats=True, **_pool_kw(mode, sampling), **KW, **kw)


@pytest.fixture(scope="module")
def ctx73(small):
    """max_batch = 7, 3 beams: two groups and one slot that is never run"""
    c = _Ctx(small, 7, 3)
    yield c
    c.e.close()


@pytest.fixture(scope="module")
def ctx42(small):
    c = _Ctx(small, 4, 2)
    yield c
    c.e.close()


def _same_as_alone(got, ref, what):
    toks, hid, score = got
    d = abs(score - ref[2])
    print(f"queue pool {what}: {len(toks)} tokens, score {score:.6f} (alone {ref[2]:.6f}, |d| {d:.3g}, tolerance "
          f"{R.tol(ref[2]):.3g}), max |d rows| {np.abs(hid - ref[1]).max() if len(toks) == len(ref[0]) and len(toks) else 0.0:.3g}")
    assert toks.tolist() == ref[0].tolist(), what
    assert d <= R.tol(ref[2]), what
    np.testing.assert_allclose(hid, ref[1], rtol=0, atol=2e-4)


def _equal(a, b):
    assert a[0].tolist() == b[0].tolist() and a[2] == b[2]           # tokens and score, bit for bit
    np.testing.assert_array_equal(a[1], b[1])


def _check_eight(ctx, mode, stops=STOPS):
    B = ctx.beams
    hosts = [ctx.host(i, mode, stops) for i in range(8)]
    margins = [min(h["margins"]) for h in hosts]
    selections = [len(h["margins"]) for h in hosts]
    print(f"queue pool, {B} beams, {mode}, stops {stops}: host-side margins {['%.3g' % m for m in margins]}, selections {selections}, "
          f"returned {[len(h['tokens']) for h in hosts]}, pool-decided {[h['from_pool_only'] for h in hosts]}, "
          f"ended by open {[h['ended_by_open'] for h in hosts]}")
    assert sum(m >= R.MARGIN for m in margins) == 8, margins        # every one of the eight is compared, none skipped
    res, stats = ctx.queue(range(8), LIMITS, mode, stops)
    assert len(res) == 8
    for i in range(8):
        _same_as_alone(res[i], ctx.alone(i, LIMITS[i], mode, stops), (B, mode, i))
        assert res[i][0].tolist() == hosts[i]["tokens"], (mode, i)
        assert abs(res[i][2] - hosts[i]["score"]) <= R.tol(hosts[i]["score"]), (mode, i)
    # the schedule the entry ran is the stated policy's over groups, on the selections each sentence ran
    steps, passes = queue_schedule([p.shape[1] for p in ctx.prompts], LIMITS, selections, ctx.cfg.max_batch, ctx.cfg.max_seq, beams=B)
    assert (stats["steps"], stats["passes"]) == (steps, len(passes))
    assert len(passes) > 2 and all(sum(1 for p in passes for _, g in p if g == u) >= 2 for u in range(ctx.cfg.max_batch // B))
    return hosts, res


@pytest.mark.parametrize("mode", list(MODES))
def test_queue_pool_3_beams_7_slots(ctx73, mode):
    hosts, res = _check_eight(ctx73, mode)
    if mode == "det":
        # the ground this stands on: lengths that are not the selections run, results only the pool could return, searches `open` ended
        assert [len(r[0]) for r in res] != [len(h["margins"]) for h in hosts]
        assert sum(h["from_pool_only"] for h in hosts) >= 3 and sum(h["ended_by_open"] for h in hosts) >= 3


@pytest.mark.parametrize("mode", list(MODES))
def test_queue_pool_2_beams_4_slots(ctx42, mode):
    _check_eight(ctx42, mode)


@pytest.mark.parametrize("mode", ["det", "sampled"])
def test_two_stop_ids(ctx73, mode):
    """K = 9 candidates per selection"""
    _check_eight(ctx73, mode, (3, 19))


def test_tenants_of_one_group(small):
    """one group (max_batch = 3, 3 beams): every sentence is the next tenant of the same pool.  Without stop ids every candidate of a
    sentence's last selection stops, so its pool ends with B finished entries; then a sentence with max_new = 1 (its pool fills at
    selection 0), then one that runs to its limit with no stop id met.  And with stop id 3: sentence 0 (7 selections, 3 tokens
    returned), the one-selection sentence 5, and two more."""
    c = _Ctx(small, 3, 3)
    try:
        for mode in ("det", "sampled"):
            for idx, limits, stops in (((0, 1, 2), [5, 1, 6], ()), ((0, 5, 1, 3), [14, 1, 9, 3], STOPS)):
                res, stats = c.queue(idx, limits, mode, stops)
                assert stats["passes"] == len(idx)
                if not stops:
                    assert [len(r[0]) for r in res] == limits
                for k, i in enumerate(idx):
                    _same_as_alone(res[k], c.alone(i, limits[k], mode, stops), ("tenant", mode, k))
    finally:
        c.e.close()


def test_sampling_depends_on_the_seed_alone(ctx73):
    e, P = ctx73.e, ctx73.prompts
    a, b = _sp(0), Sampling(1.0, 30, 0.8, 77)
    # sentence 0 twice with one seed: the first copy in group 0 by pass 0; sentence 5 (limit 1) frees group 1 right after that pass,
    # so the second copy is admitted by pass 1 into group 1 while the first is still decoding
    res, stats = ctx73.queue((0, 5, 0), [14, 1, 14], "sampled", sampling=[a, _sp(5), a])
    assert stats["passes"] == 2
    _equal(res[0], res[2])
    _same_as_alone(res[0], ctx73.alone(0, 14, "sampled"), "twin")    # and what the sentence gives alone
    # two seeds
    two, _ = ctx73.queue((0, 0), [14, 14], "sampled", sampling=[a, b])
    _equal(two[0], res[0])
    assert two[0][0].tolist() != two[1][0].tolist() or two[0][2] != two[1][2]
    # the whole call twice (the captured graphs by now), then eagerly (profiling: eager launches)
    x, sx = ctx73.queue(range(8), LIMITS, "sampled")
    y, sy = ctx73.queue(range(8), LIMITS, "sampled")
    _lib.prof_reset(); _lib.prof_enable(("attn",))
    try:
        z, sz = ctx73.queue(range(8), LIMITS, "sampled")
        zd, _ = ctx73.queue(range(8), LIMITS, "det")
    finally:
        _lib.prof_enable(())
    assert sx == sy == sz
    d, _ = ctx73.queue(range(8), LIMITS, "det")
    for i in range(8):
        _equal(x[i], y[i])
        _equal(x[i], z[i])
        _equal(d[i], zd[i])


def _host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("mode", ["det", "sampled"])
def test_session(ctx73, mode, device):
    """count is 0 or n_out and never in between; tokens, rows and score leave in the round that retires the sentence; the final
    arrays and scores are the blocking entry's, bit for bit (device=True: MI_DEVICE arrays give what MI_HOST gives)"""
    e, P = ctx73.e, ctx73.prompts
    idx, limits = list(range(8)) + [0], LIMITS + [0]
    samp = ctx73.samplings(mode, idx)
    res, stats = ctx73.queue(idx, limits, mode, sampling=samp)
    n_out = np.asarray([len(r[0]) for r in res])
    assert n_out[8] == 0 and res[8][2] == 0.0 and (n_out[:8] >= 1).all()
    with e.queue_session([P[i] for i in idx], limits, stop_tokens=list(STOPS), beams=3, device=device, **_pool_kw(mode, samp), **KW) as q:
        finished, rounds, prev_d = False, 0, np.zeros(9, bool)
        while not finished:
            count, done, finished = q.advance()
            rounds += 1
            assert rounds < 200
            assert np.all((count == 0) | (count == n_out)), count      # never in between
            assert np.all(done == np.where(n_out > 0, count == n_out, True)) and np.all(done >= prev_d)
            assert finished == bool(np.all(done))
            tk, hd, sc = _host(q.tokens), _host(q.hidden), _host(q.scores)
            for i in np.nonzero(done)[0]:
                np.testing.assert_array_equal(tk[i, : count[i]], res[i][0])      # tokens, rows (final) and score leave in that round
                np.testing.assert_array_equal(hd[i, : count[i]], res[i][1])
                assert sc[i] == np.float32(res[i][2])
            prev_d = done
        again = q.advance()
        assert again[2] and np.array_equal(again[0], count)
        assert q.stats == stats and rounds > 2 and count.tolist() == n_out.tolist()
    after, _ = ctx73.queue(idx, limits, mode, sampling=samp)
    for a, b in zip(after, res):
        _equal(a, b)


def _raw_args(e, prompts, limits, cap):
    cfg = e.cfg
    cat = np.ascontiguousarray(np.concatenate([p.reshape(-1, cfg.hidden) for p in prompts]), np.float32)
    rows = np.ascontiguousarray([p.shape[1] for p in prompts], np.int32)
    mx = np.ascontiguousarray(limits, np.int32)
    n = len(prompts)
    return cat, rows, mx, np.zeros((n, cap), np.int32), np.zeros((n, cap, cfg.hidden), np.float32), np.zeros(n, np.int32), \
        np.zeros(n, np.float32)


def test_session_estate_and_end_midway(small, ctx73):
    e, P = ctx73.e, ctx73.prompts
    L = _lib.load()
    fresh = _engine(small, 7)                                         # an alone pool call as the first call on a handle
    want, _ = fresh.generate_beam([P[0]], [14], 3, stop_tokens=list(STOPS), **_pool_kw("sampled", _sp(0)), **KW)
    fresh.close()
    ref, _ = ctx73.queue(range(8), LIMITS, "sampled")
    q = e.queue_session(P, LIMITS, stop_tokens=list(STOPS), beams=3, **_pool_kw("sampled", ctx73.samplings("sampled")), **KW)
    count, done, finished = q.advance()
    assert not finished
    cat, rows, mx, toks, hid, n_out, sc = _raw_args(e, P[:2], [3, 3], 3)
    assert L.mi_gpt_queue_begin_beam_pool(e._h, 2, cat.ctypes.data, _lib.i32p(rows), _lib.i32p(mx), None, 0, 0.7, 3, 3, 0.0, 0, None,
                                          None, None, None, toks.ctypes.data, hid.ctypes.data, 3, sc.ctypes.data,
                                          _lib.MI_HOST) == MI_ESTATE
    assert L.mi_gpt_generate_queue_beam_pool(e._h, 2, cat.ctypes.data, _lib.i32p(rows), _lib.i32p(mx), None, 0, 0.7, 3, 3, 0.0, 0,
                                             None, None, None, None, toks.ctypes.data, hid.ctypes.data, 3, _lib.i32p(n_out),
                                             sc.ctypes.data, _lib.MI_HOST, None) == MI_ESTATE
    assert L.mi_gpt_generate_beam_pool(e._h, 2, cat.ctypes.data, _lib.i32p(rows), _lib.i32p(mx), None, 0, 0.7, 3, None, 3, 0.0, 0,
                                       None, None, None, None, toks.ctypes.data, hid.ctypes.data, 3, _lib.i32p(n_out), None,
                                       _lib.MI_HOST) == MI_ESTATE
    last, tok, logits = np.zeros((1, e.cfg.hidden), np.float32), np.zeros(1, np.int32), np.zeros((1, e.cfg.mel_codes), np.float32)
    assert L.mi_gpt_step(e._h, cat.ctypes.data, 1, None, 1, last.ctypes.data, tok.ctypes.data, logits.ctypes.data,
                         _lib.MI_HOST) == MI_ESTATE
    assert b"session" in L.mi_last_error()
    count2, done2, _ = q.advance()                                   # the session went on undisturbed
    assert done2.any()
    for i in np.nonzero(done2)[0]:
        np.testing.assert_array_equal(q.tokens[i, : count2[i]], ref[i][0])
        np.testing.assert_array_equal(q.hidden[i, : count2[i]], ref[i][1])
        assert q.scores[i] == np.float32(ref[i][2])
    q.end()                                                          # mid-way
    assert L.mi_gpt_queue_end(e._h) == MI_ESTATE
    got, _ = e.generate_beam([P[0]], [14], 3, stop_tokens=list(STOPS), **_pool_kw("sampled", _sp(0)), **KW)
    _equal(got[0], want[0])


def test_einval_leaves_the_handle_usable(small, ctx73):
    e, P = ctx73.e, ctx73.prompts
    cfg = e.cfg
    L = _lib.load()
    good, _ = ctx73.queue(range(3), LIMITS[:3], "sampled")
    stops6 = np.arange(6, dtype=np.int32)
    T, K, TP, S = (np.full(3, 1.0, np.float32), np.full(3, 30, np.int32), np.full(3, 0.8, np.float32),
                   np.arange(3, dtype=np.uint64) + 1001)
    sa = (T, K, TP, S)

    def args(eng, beams, limits, cap, prompts, n_stop, lp, es, samp):
        cat, rows, mx, toks, hid, n, sc = _raw_args(eng, prompts, limits, cap)
        keep = (cat, rows, mx, toks, hid, n, sc)
        head = (eng._h, len(prompts), cat.ctypes.data, _lib.i32p(rows), _lib.i32p(mx), stops6.ctypes.data if n_stop else None, n_stop,
                0.7, 3, beams, lp, es, *(None if a is None else a.ctypes.data for a in samp))
        return keep, head, toks, hid, cap, n, sc

    def call(beams=3, limits=LIMITS[:3], cap=16, prompts=P[:3], n_stop=1, lp=0.0, es=0, samp=(None,) * 4, eng=e):
        keep, head, toks, hid, cap, n, sc = args(eng, beams, limits, cap, prompts, n_stop, lp, es, samp)
        return L.mi_gpt_generate_queue_beam_pool(*head, toks.ctypes.data, hid.ctypes.data, cap, _lib.i32p(n), sc.ctypes.data,
                                                 _lib.MI_HOST, None)

    def begin(beams=3, limits=LIMITS[:3], cap=16, prompts=P[:3], n_stop=1, lp=0.0, es=0, samp=(None,) * 4, eng=e):
        keep, head, toks, hid, cap, n, sc = args(eng, beams, limits, cap, prompts, n_stop, lp, es, samp)
        return L.mi_gpt_queue_begin_beam_pool(*head, toks.ctypes.data, hid.ctypes.data, cap, sc.ctypes.data, _lib.MI_HOST)

    assert call() == 0 and call(samp=sa) == 0
    longp = _prompt(e, 9, 22)
    assert longp.shape[1] + 37 - 1 == cfg.max_seq + 1 and 37 <= cfg.max_mel_pos
    assert cfg.max_batch + 1 <= 8                                     # a num_beams within [1, 8] and above max_batch
    bad = [dict(beams=0), dict(beams=9), dict(beams=cfg.max_batch + 1),                                  # num_beams
           dict(limits=[4, 17, 4]), dict(limits=[4, -1, 4]), dict(limits=[4, cfg.max_mel_pos + 1, 4], cap=64),      # lengths per sentence
           dict(limits=[3, 3, 37], cap=40, prompts=[P[0], P[1], longp]),
           dict(lp=float("nan")), dict(lp=float("inf")), dict(es=2), dict(es=-1),
           dict(samp=(T, None, None, None)), dict(samp=(T, K, TP, None)),                                 # only some of the four arrays
           dict(samp=(np.array([1.0, 0.0, 1.0], np.float32), K, TP, S)),                                  # invalid records
           dict(samp=(T, K, np.array([0.8, 0.8, 1.5], np.float32), S)),
           dict(samp=(T, np.array([30, -1, 30], np.int32), TP, S)),
           dict(n_stop=3, samp=(T, np.array([30, 8, 30], np.int32), TP, S))]                              # top_k = 8 below K = 12
    for b in bad:
        assert call(**b) == _lib.MI_EINVAL, b
        assert begin(**b) == _lib.MI_EINVAL, b
        assert L.mi_gpt_queue_end(e._h) == MI_ESTATE                  # no session was left open
    again, _ = ctx73.queue(range(3), LIMITS[:3], "sampled")           # the handle still decodes, and the same
    for a, b in zip(again, good):
        _equal(a, b)
    # K = (n_stop + 1) * num_beams above the 50 mel codes (8 beams need max_batch = 8), and more than 16384 codes with sampling
    e8 = _engine(small, 8)
    P8 = [_prompt(e8, 1 + b, TEXT[b]) for b in range(3)]
    assert call(beams=8, n_stop=6, prompts=P8, eng=e8) == _lib.MI_EINVAL and begin(beams=8, n_stop=6, prompts=P8, eng=e8) == _lib.MI_EINVAL
    assert call(beams=8, n_stop=5, prompts=P8, eng=e8) == 0           # K = 48 fits
    e8.close()
    wide = IndexGPTConfig(hidden=128, layers=1, heads=2, inner=256, mel_codes=16385, text_tokens=64, max_mel_pos=32, max_text_pos=32,
                          max_seq=32, max_batch=3, start_mel_token=16383, stop_mel_token=16384)
    ew = IndexGPT(wide, W.synth_state(W.gpt_spec(wide), 3), dtype="f32")
    Pw = [_prompt(ew, 1 + b, 3) for b in range(3)]
    assert call(limits=[2, 2, 2], prompts=Pw, samp=sa, eng=ew) == _lib.MI_EINVAL
    assert begin(limits=[2, 2, 2], prompts=Pw, samp=sa, eng=ew) == _lib.MI_EINVAL
    assert call(limits=[2, 2, 2], prompts=Pw, eng=ew) == 0            # deterministic pool mode has no such limit
    ew.close()
    with pytest.raises(ValueError):
        e.generate_queue(P[:3], LIMITS[:3], pool=True)                # pool mode is a beam mode
    with pytest.raises(ValueError):
        e.queue_session(P[:3], LIMITS[:3], pool=True, sampling=_sp(1))
    with pytest.raises(ValueError):
        e.generate_queue(P[:3], LIMITS[:3], beams=2, sampling=_sp(1))     # sampling with beams needs the pool
    with pytest.raises(ValueError):
        e.queue_session(P[:3], LIMITS[:3], beams=2, sampling=_sp(1))
    with pytest.raises(ValueError):
        e.generate_queue(P[:3], LIMITS[:3], beams=3, pool=True, sampling=Sampling(1.0, 4, 0.8, 1))      # top_k 4 below K = 6 (MI_EINVAL)


def test_edges(small, ctx73):
    e, P = ctx73.e, ctx73.prompts
    cfg = e.cfg
    for mode in ("det", "sampled"):
        # n smaller than the group count: one pass, nothing refilled
        one, stats = ctx73.queue((2,), [7], mode)
        _same_as_alone(one[0], ctx73.alone(2, 7, mode), ("n=1", mode))
        assert stats["passes"] == 1
        # a sentence with max_new = 0 between two others: no group, nothing returned, score 0
        res, stats = ctx73.queue((0, 1, 2), [LIMITS[0], 0, LIMITS[2]], mode)
        assert len(res[1][0]) == 0 and res[1][1].shape == (0, cfg.hidden) and res[1][2] == 0.0 and stats["passes"] == 1
        _same_as_alone(res[0], ctx73.alone(0, LIMITS[0], mode), ("around 0", mode))
        _same_as_alone(res[2], ctx73.alone(2, LIMITS[2], mode), ("around 0", mode))
    res, stats = ctx73.queue((0, 1), [0, 0], "det")
    assert [len(r[0]) for r in res] == [0, 0] and [r[2] for r in res] == [0.0, 0.0] and stats == {"steps": 0, "passes": 0}
    # 1 beam, deterministic, length_penalty 0: the tokens of the greedy queue (7 groups of one slot)
    for stops in ((), STOPS):
        g = e.generate_queue(P, LIMITS, stop_tokens=list(stops), **KW)
        b1 = e.generate_queue(P, LIMITS, stop_tokens=list(stops), beams=1, pool=True, **KW)
        for i in range(8):
            assert b1[i][0].tolist() == g[i][0].tolist(), (stops, i)
            np.testing.assert_allclose(b1[i][1], g[i][1], rtol=0, atol=2e-4)
    # 8 beams on max_batch = 8: one group, K = 16 with one stop id
    c8 = _Ctx(small, 8, 8)
    try:
        for mode in ("det", "sampled"):
            idx, limits = (0, 5, 2, 3), [LIMITS[0], 1, LIMITS[2], LIMITS[3]]
            res, stats = c8.queue(idx, limits, mode)
            assert stats["passes"] == 4
            for k, i in enumerate(idx):
                _same_as_alone(res[k], c8.alone(i, limits[k], mode), ("8 beams", mode, k))
    finally:
        c8.e.close()


def test_blocking_entry_on_device_arrays(ctx73):
    import torch
    e, P = ctx73.e, ctx73.prompts
    idx, limits = list(range(8)) + [0], LIMITS + [0]
    ref, _ = ctx73.queue(idx, limits, "det")
    cat, rows, mx, toks, hid, n_out, sc = _raw_args(e, [P[i] for i in idx], limits, max(LIMITS))
    dev = torch.device("cuda", e.device)
    d_cat = torch.from_numpy(cat).to(dev)
    d_stop = torch.tensor(list(STOPS), dtype=torch.int32, device=dev)
    d_tok = torch.zeros(toks.shape, dtype=torch.int32, device=dev)
    d_hid = torch.zeros(hid.shape, dtype=torch.float32, device=dev)
    d_sc = torch.full(sc.shape, 5.0, dtype=torch.float32, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    rc = _lib.load().mi_gpt_generate_queue_beam_pool(e._h, 9, d_cat.data_ptr(), _lib.i32p(rows), _lib.i32p(mx), d_stop.data_ptr(), 1,
                                                     0.7, 3, 3, 0.0, 0, None, None, None, None, d_tok.data_ptr(), d_hid.data_ptr(),
                                                     max(LIMITS), _lib.i32p(n_out), d_sc.data_ptr(), _lib.MI_DEVICE, None)
    assert rc == 0 and n_out.tolist() == [len(r[0]) for r in ref]
    tk, hd, s = d_tok.cpu().numpy(), d_hid.cpu().numpy(), d_sc.cpu().numpy()
    for i in range(9):
        _equal((tk[i, : n_out[i]], hd[i, : n_out[i]], float(s[i])), ref[i])


def _lead(margins, bound):
    k = 0
    while k < len(margins) and margins[k] >= bound:
        k += 1
    return k


@pytest.mark.parametrize("dtype,eps", [("f16", 2.0 ** -11), ("bf16", 2.0 ** -8)])
def test_16_bit_engines(small, dtype, eps):
    """The eight sentences on the 16-bit engines: codes in range, finite rows and scores; one pool beam gives the greedy queue's
    tokens exactly (both read the batched step and the packed pass).  And a case against the engine's own host-driven loop, by
    the decision rule of test_pool_16_bit_engines (tests/test_gpu_gpt_beam_pool.py): that loop reads its logits from the
    single-sentence step, the queue from the packed pass and the batched step, kernels that round the same 16-bit activations in
    different places, so a logit may differ by d = eps * zmax (eps = half an ulp of the format, zmax = the largest |logits * pen|
    the host-driven loop read) and a log-probability by 2 d; a selection is decided when its host-side margin is at least 4 d.
    Per mode the case is searched on the host-driven loop alone, over sentences 0-5 and two, one and no stop id at 3 beams: the
    run with the most decided leading selections, cut to that many selections (max_new) and cut further until every selection of
    the cut run is decided.  That case must exist; it goes through the queue as the third of three sentences, so into a refilled
    group, and must give the host-driven tokens, and its score to len(tokens) * 2 d."""
    c = _Ctx(small, 7, 3)
    c.e.close()
    c.e = e = _engine(small, 7, dtype)
    c.prompts = P = [_prompt(e, 1 + b, TEXT[b]) for b in range(8)]
    try:
        for mode in ("det", "sampled"):
            res, _ = c.queue(range(8), LIMITS, mode)
            for i, (toks, hid, score) in enumerate(res):
                assert 1 <= len(toks) <= LIMITS[i] and toks.min() >= 0 and toks.max() < e.cfg.mel_codes
                assert np.isfinite(hid).all() and np.isfinite(score) and score < 0.0
        for stops in ((), STOPS):
            one = e.generate_queue(P, LIMITS, stop_tokens=list(stops), beams=1, pool=True, **KW)
            g = e.generate_queue(P, LIMITS, stop_tokens=list(stops), **KW)
            for i in range(8):
                assert one[i][0].tolist() == g[i][0].tolist(), i

        def host(i, stops, sampled, max_new):
            sp = _sp(i)
            return R.pool_generate(RB.EngineModel(e), P[i], 3, max_new, stop_tokens=stops, length_penalty=0.0,
                                   sampling=dict(temperature=sp.temperature, top_k=sp.top_k, top_p=sp.top_p, seed=sp.seed)
                                   if sampled else None, **KW)

        for mode, sampled in (("det", False), ("sampled", True)):
            best = None
            for i in range(6):
                for stops in ((3, 19), STOPS, ()):
                    ref = host(i, stops, sampled, LIMITS[i])
                    k = _lead(ref["margins"], 4 * eps * ref["zmax"])
                    if best is None or k > best[0]:
                        best = (k, i, stops, len(ref["margins"]))
            k, i, stops, n_sel = best
            m = LIMITS[i] if k == n_sel else k
            ref = None
            while m >= 1:
                ref = host(i, stops, sampled, m)
                d = eps * ref["zmax"]
                if min(ref["margins"]) >= 4 * d:
                    break
                m, ref = m - 1, None
            assert ref is not None, (dtype, mode, best)               # a case decided throughout exists
            others = [j for j in range(8) if j != i][:2]
            lp = 0.0
            got = e.generate_queue([P[others[0]], P[others[1]], P[i]], [2, 9, m], stop_tokens=list(stops), beams=3, pool=True,
                                   length_penalty=lp, sampling=[_sp(others[0]), _sp(others[1]), _sp(i)] if sampled else None, **KW)
            toks, hid, score = got[2]
            print(f"queue pool {dtype} {mode}: sentence {i}, {len(stops)} stop ids, max_new {m}: {len(toks)} tokens, min margin "
                  f"{min(ref['margins']):.3g}, 4 d = {4 * d:.3g}, score {score:.6f} / {ref['score']:.6f}")
            assert toks.tolist() == ref["tokens"], (dtype, mode)
            assert abs(score - ref["score"]) <= len(toks) * 2 * d + R.tol(ref["score"]), (dtype, mode)
            assert hid.shape == ref["hidden"].shape and np.isfinite(hid).all()
    finally:
        e.close()
