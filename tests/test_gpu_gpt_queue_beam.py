"""GPU: beam search through the sentence queue (mi_gpt_generate_queue_beam / mi_gpt_queue_begin_beam; IndexGPT.generate_queue and
queue_session with ``beams``): a sentence runs as a group of B consecutive slots, the queue schedules groups, the prompts admitted
together run as one packed pass with selection 0 of all their groups in one launch, and a finished group leaves along its
ancestor table ahead of the pass that refills it.

Per sentence the result has to be what mi_gpt_generate_beam gives for that sentence alone from a penalty vector of ones: the decode
steps are the same launches and the packed prompt pass differs from the one-by-one pass in GEMM tiling (fp32: summation order)
only.  Bars, all the project's own: tokens equal; |score difference| <= gpt_beam_ref.tol; rows within 2e-4 of the engine's alone
run and within 3e-4 of the numpy oracle.  Tokens are compared where rounding cannot decide: the host-driven margin (the smallest
gap among the sorted top B + 1 candidates over all selections, tests/gpt_beam_ref.py) of every one of the eight sentences has to be
at least MARGIN = 1e-4 (tests/test_gpu_gpt_beam.py), and the oracle comparison takes the sentences whose oracle-side margin is at
least the oracle gate 6 x 4 x 3e-4 of test_device_beam_vs_oracle: at 3 beams sentences 1, 2, 3, 5, 6 and 7 (>= 7.67e-3; sentence 0
has 2.9e-3 and sentence 4 has 1.15e-3).  The entry's stats are held against queue_schedule(..., beams=B)."""
import numpy as np
import pytest

import gpt_beam_ref as R
from mi355tts import weights as W
from mi355tts import _lib
from mi355tts.config import IndexGPTConfig
from mi355tts.indextts import IndexGPT, Sampling, lockstep_steps, queue_schedule

pytestmark = pytest.mark.gpu
SEED = 9527
MARGIN = 1e-4             # host-side margin from which a decode case is compared in full (tests/test_gpu_gpt_beam.py)
ORACLE_GATE = 6 * 4 * 3e-4
KW = dict(repeat_value=0.7, penalty_range=3)
TEXT = (6, 3, 9, 5, 1, 8, 4, 7)
LIMITS = [14, 9, 11, 3, 12, 1, 10, 6]
MI_ESTATE = -4            # include/mi355tts.h


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


class _Ctx:
    """an engine, the eight sentences, and every sentence's alone run (mi_gpt_generate_beam, one group) by stop ids, once each"""

    def __init__(self, small, max_batch, beams):
        self.e = _engine(small, max_batch)
        self.cfg, self.beams = self.e.cfg, beams
        self.prompts = [_prompt(self.e, 1 + b, TEXT[b]) for b in range(8)]
        self._alone, self._host = {}, {}

    def alone(self, i, limit, stops=()):
        key = (i, limit, tuple(stops))
        if key not in self._alone:
            res, _ = self.e.generate_beam([self.prompts[i]], [limit], self.beams, stop_tokens=list(stops), **KW)
            self._alone[key] = res[0]
        return self._alone[key]

    def host(self, i, stops=()):
        """the definition's loop over the engine's own single-sentence step (every hypothesis with its own cache copy)"""
        key = (i, tuple(stops))
        if key not in self._host:
            self._host[key] = R.beam_generate(R.EngineModel(self.e), self.prompts[i], self.beams, LIMITS[i], stop_tokens=stops, **KW)
        return self._host[key]

    def model(self, prompts, limits, res):
        steps, passes = queue_schedule([p.shape[1] for p in prompts], limits, [len(r[0]) for r in res], self.cfg.max_batch,
                                       self.cfg.max_seq, beams=self.beams)
        return steps, passes


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


_ORACLE = {}


def _oracle(small, ctx, i):
    key = (ctx.beams, i)
    if key not in _ORACLE:
        cfg, st = small
        _ORACLE[key] = R.beam_generate(R.OracleModel(cfg, st), ctx.prompts[i], ctx.beams, LIMITS[i], **KW)
    return _ORACLE[key]


def _same_as_alone(got, ref, what):
    toks, hid, score = got
    d = abs(score - ref[2])
    print(f"queue beam {what}: {len(toks)} tokens, score {score:.6f} (alone {ref[2]:.6f}, |d| {d:.3g}, tolerance "
          f"{R.tol(ref[2]):.3g}), max |d rows| {np.abs(hid - ref[1]).max() if len(toks) == len(ref[0]) and len(toks) else 0.0:.3g}")
    assert toks.tolist() == ref[0].tolist(), what
    assert d <= R.tol(ref[2]), what
    np.testing.assert_allclose(hid, ref[1], rtol=0, atol=2e-4)


def _equal(a, b):
    assert a[0].tolist() == b[0].tolist() and a[2] == b[2]           # tokens and score, bit for bit
    np.testing.assert_array_equal(a[1], b[1])


def _check_eight(small, ctx, oracle_set):
    e, B = ctx.e, ctx.beams
    margins = [min(ctx.host(i)["margins"]) for i in range(8)]
    print(f"queue beam, {B} beams: host-side margins {['%.3g' % m for m in margins]}")
    assert sum(m >= MARGIN for m in margins) == 8, margins          # every one of the eight is compared, none skipped
    res, stats = e.generate_queue(ctx.prompts, LIMITS, stop_tokens=[], beams=B, return_stats=True, **KW)
    assert len(res) == 8 and [len(r[0]) for r in res] == LIMITS
    for i in range(8):
        _same_as_alone(res[i], ctx.alone(i, LIMITS[i]), (B, i))
        host = ctx.host(i)
        assert res[i][0].tolist() == host["tokens"] and abs(res[i][2] - host["score"]) <= R.tol(host["score"]), i
    compared = []
    for i in range(8):
        ref = _oracle(small, ctx, i)
        m = min(ref["margins"])
        if i not in oracle_set:
            print(f"queue beam vs oracle ({B}, {i}): oracle margin {m:.3g}, below the gate {ORACLE_GATE:.3g}: engine only")
            assert m < ORACLE_GATE
            continue
        assert m >= ORACLE_GATE, (i, m)
        compared.append(i)
        print(f"queue beam vs oracle ({B}, {i}): margin {m:.3g}, max |d rows| {np.abs(res[i][1] - ref['hidden']).max():.3g}")
        assert res[i][0].tolist() == ref["tokens"], i
        np.testing.assert_allclose(res[i][1], ref["hidden"], rtol=0, atol=3e-4)
    # the schedule the entry ran is the stated policy's over groups, on the lengths it produced
    steps, passes = ctx.model(ctx.prompts, LIMITS, res)
    assert (stats["steps"], stats["passes"]) == (steps, len(passes))
    assert len(passes) > 1
    return compared


def test_queue_beam_3_beams_7_slots(small, ctx73):
    assert _check_eight(small, ctx73, (1, 2, 3, 5, 6, 7)) == [1, 2, 3, 5, 6, 7]


def test_queue_beam_2_beams_4_slots(small, ctx42):
    """at 2 beams the oracle-side margins of sentences 0 and 1 are 2.9e-3 and 1.06e-3, below the gate; the other six have at least
    7.67e-3 and are compared against the oracle"""
    assert _check_eight(small, ctx42, (2, 3, 4, 5, 6, 7)) == [2, 3, 4, 5, 6, 7]


def test_stop_id_ends_a_group_and_it_is_refilled_at_once(ctx73):
    e = ctx73.e
    stop = ctx73.host(0)["top_tokens"][4]                             # hypothesis 0's token after selection 4 of sentence 0
    assert stop == 7                                                  # what it is on the numpy oracle
    res, stats = e.generate_queue(ctx73.prompts, LIMITS, stop_tokens=[stop], beams=3, return_stats=True, **KW)
    assert len(res[0][0]) == 5 and res[0][0][-1] == stop
    for i in range(8):
        _same_as_alone(res[i], ctx73.alone(i, LIMITS[i], (stop,)), ("stop", i))
    steps, passes = ctx73.model(ctx73.prompts, LIMITS, res)
    assert (stats["steps"], stats["passes"]) == (steps, len(passes))
    # the model with sentence 0 ending after 5 tokens, against the same model with it running to its limit: it frees group 0
    # at the end of the first run of steps, and the pass that refills group 0 comes with no decode step in between (a run of
    # steps never splits: the step count of the schedule up to that pass is the first run's)
    first_refill = next(p for p in passes[1:] if any(g == 0 for _, g in p))
    assert first_refill[0][0] == 2                                    # sentence 2 is the next in index order


def test_schedule_is_real():
    """Two groups of 3 beams in 6 slots, limits [65, 17, 17, 17, 17], no stop ids: 64 decode steps in 4 passes (index-order groups
    of two sentences need 96)."""
    cfg = IndexGPTConfig(hidden=256, layers=2, heads=4, inner=1024, mel_codes=301, text_tokens=64, max_mel_pos=80,
                         max_text_pos=80, max_seq=96, max_batch=6, start_mel_token=299, stop_mel_token=300)
    st = W.synth_state(W.gpt_spec(cfg), 11)
    e = IndexGPT(cfg, st, dtype="f32")
    prompts = [_prompt(e, 10 + b, 3 + (b * 7) % 11, n_cond=8) for b in range(5)]
    limits = [65, 17, 17, 17, 17]
    res, stats = e.generate_queue(prompts, limits, stop_tokens=[], beams=3, return_stats=True, **KW)
    assert [len(r[0]) for r in res] == limits
    assert (stats["steps"], stats["passes"]) == (64, 4)
    steps, passes = queue_schedule([p.shape[1] for p in prompts], limits, limits, cfg.max_batch, cfg.max_seq, beams=3)
    assert (steps, len(passes)) == (64, 4) and lockstep_steps(limits, cfg.max_batch // 3) == 96
    for b in (0, 4):
        alone, _ = e.generate_beam([prompts[b]], [limits[b]], 3, stop_tokens=[], **KW)
        assert res[b][0].tolist() == alone[0][0].tolist(), b
        np.testing.assert_allclose(res[b][1], alone[0][1], rtol=0, atol=2e-4)
        assert abs(res[b][2] - alone[0][2]) <= R.tol(alone[0][2])
    e.close()


def _raw_args(e, prompts, limits, cap):
    cfg = e.cfg
    cat = np.ascontiguousarray(np.concatenate([p.reshape(-1, cfg.hidden) for p in prompts]), np.float32)
    rows = np.ascontiguousarray([p.shape[1] for p in prompts], np.int32)
    mx = np.ascontiguousarray(limits, np.int32)
    n = len(prompts)
    return cat, rows, mx, np.zeros((n, cap), np.int32), np.zeros((n, cap, cfg.hidden), np.float32), np.zeros(n, np.int32), \
        np.zeros(n, np.float32)


def test_edges(ctx73):
    e, P = ctx73.e, ctx73.prompts
    cfg = e.cfg
    # n <= G: one pass, nothing refilled
    res, stats = e.generate_queue(P[:2], LIMITS[:2], stop_tokens=[], beams=3, return_stats=True, **KW)
    assert stats == {"steps": 13, "passes": 1}
    for i in range(2):
        _same_as_alone(res[i], ctx73.alone(i, LIMITS[i]), ("n<=G", i))
    # n = 1
    one, stats = e.generate_queue(P[2:3], [7], stop_tokens=[], beams=3, return_stats=True, **KW)
    _same_as_alone(one[0], ctx73.alone(2, 7), "n=1")
    assert stats == {"steps": 6, "passes": 1}
    # max_new of 0 and of 1: no group and n_out = 0; one token right after the prompt pass
    res, stats = e.generate_queue(P[:4], [0, 1, 5, 0], stop_tokens=[], beams=3, return_stats=True, **KW)
    assert [len(r[0]) for r in res] == [0, 1, 5, 0] and res[0][1].shape == (0, cfg.hidden)
    _same_as_alone(res[1], ctx73.alone(1, 1), "limit 1")
    _same_as_alone(res[2], ctx73.alone(2, 5), "limit 5")
    assert stats == {"steps": 4, "passes": 1}
    res, stats = e.generate_queue(P[:2], [0, 0], stop_tokens=[], beams=3, return_stats=True, **KW)
    assert [len(r[0]) for r in res] == [0, 0] and stats == {"steps": 0, "passes": 0}
    # a sentence whose token 0 is the stop id: its group retires after its prompt pass and the next sentence takes it at once
    stop0 = int(ctx73.alone(1, 1)[0][0])          # hypothesis 0's token after selection 0 (not token 0 of the final path)
    four = [0, 1, 2, 0]
    res, stats = e.generate_queue([P[i] for i in four], [6] * 4, stop_tokens=[stop0], beams=3, return_stats=True, **KW)
    assert res[1][0].tolist() == [stop0]
    for k, i in enumerate(four):
        _same_as_alone(res[k], ctx73.alone(i, 6, (stop0,)), ("token 0 stops", k))
    steps, passes = ctx73.model([P[i] for i in four], [6] * 4, res)
    assert passes[0] == [(0, 0), (1, 1)] and passes[1][0] == (2, 1) and (stats["steps"], stats["passes"]) == (steps, len(passes))
    # beams = 1 against the greedy queue
    g = e.generate_queue(P, LIMITS, stop_tokens=[], **KW)
    b1, stats1 = e.generate_queue(P, LIMITS, stop_tokens=[], beams=1, return_stats=True, **KW)
    for i in range(8):
        assert b1[i][0].tolist() == g[i][0].tolist(), i
        np.testing.assert_allclose(b1[i][1], g[i][1], rtol=0, atol=2e-4)
    sched = queue_schedule([p.shape[1] for p in P], LIMITS, LIMITS, cfg.max_batch, cfg.max_seq)
    assert (stats1["steps"], stats1["passes"]) == (sched[0], len(sched[1]))
    # a pass cut by max_seq packed rows: two 37-row prompts do not share the 64-row scratch
    long_a, long_b = _prompt(e, 21, 22, n_cond=12), _prompt(e, 22, 22, n_cond=12)
    assert long_a.shape[1] == 37 and 2 * 37 > cfg.max_seq
    cut = [long_a, long_b, P[0]]
    res, stats = e.generate_queue(cut, [3, 3, 3], stop_tokens=[], beams=3, return_stats=True, **KW)
    assert queue_schedule([37, 37, P[0].shape[1]], [3] * 3, [3] * 3, cfg.max_batch, cfg.max_seq, beams=3) == \
        (stats["steps"], [[(0, 0)], [(1, 1)], [(2, 0)]])
    assert stats["passes"] == 3
    for k, p in enumerate(cut):
        alone, _ = e.generate_beam([p], [3], 3, stop_tokens=[], **KW)
        _same_as_alone(res[k], alone[0], ("cut", k))


def test_einval_leaves_the_handle_usable(ctx73):
    e, P = ctx73.e, ctx73.prompts
    cfg = e.cfg
    L = _lib.load()
    good = e.generate_queue(P[:3], LIMITS[:3], stop_tokens=[], beams=3, **KW)

    def call(beams, limits, cap=16, prompts=P[:3]):
        cat, rows, mx, toks, hid, n, sc = _raw_args(e, prompts, limits, cap)
        return L.mi_gpt_generate_queue_beam(e._h, len(prompts), cat.ctypes.data, _lib.i32p(rows), _lib.i32p(mx), None, 0, 0.7, 3,
                                            beams, toks.ctypes.data, hid.ctypes.data, cap, _lib.i32p(n), sc.ctypes.data,
                                            _lib.MI_HOST, None)

    def begin(beams, limits, cap=16):
        cat, rows, mx, toks, hid, n, sc = _raw_args(e, P[:3], limits, cap)
        return L.mi_gpt_queue_begin_beam(e._h, 3, cat.ctypes.data, _lib.i32p(rows), _lib.i32p(mx), None, 0, 0.7, 3, beams,
                                         toks.ctypes.data, hid.ctypes.data, cap, sc.ctypes.data, _lib.MI_HOST)

    longp = _prompt(e, 9, 22)
    assert longp.shape[1] + 37 - 1 == cfg.max_seq + 1 and 37 <= cfg.max_mel_pos
    cases = [(0, LIMITS[:3], {}), (9, LIMITS[:3], {}), (cfg.max_batch + 1, LIMITS[:3], {}),      # num_beams
             (3, [4, 17, 4], {}), (3, [4, -1, 4], {}), (3, [4, cfg.max_mel_pos + 1, 4], {"cap": 64}),      # limits out of range
             (3, [3, 3, 37], {"cap": 40, "prompts": [P[0], P[1], longp]})]
    assert cfg.max_batch + 1 <= 8                                     # the third case is within [1, 8] and above max_batch
    for beams, limits, kw in cases:
        assert call(beams, limits, **kw) == _lib.MI_EINVAL, (beams, limits)
        again = e.generate_queue(P[:3], LIMITS[:3], stop_tokens=[], beams=3, **KW)
        for a, b in zip(again, good):
            _equal(a, b)
    for beams, limits in ((0, LIMITS[:3]), (9, LIMITS[:3]), (3, [4, 17, 4])):
        assert begin(beams, limits) == _lib.MI_EINVAL
        assert L.mi_gpt_queue_end(e._h) == MI_ESTATE                  # no session was left open
    with pytest.raises(ValueError):
        e.generate_queue(P[:3], LIMITS[:3], beams=2, sampling=Sampling(seed=1))
    with pytest.raises(ValueError):
        e.queue_session(P[:3], LIMITS[:3], beams=2, sampling=Sampling(seed=1))
    with pytest.raises(ValueError):
        e.generate_queue(P[:3], LIMITS[:3], beams=8)                  # one group does not fit max_batch = 7


def _host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_session(ctx73, device):
    """count is 0 or n_out and never in between; the final arrays and scores are the blocking entry's, bit for bit (device=True:
    MI_DEVICE arrays give what MI_HOST gives)"""
    e, P = ctx73.e, ctx73.prompts
    stop = ctx73.host(0)["top_tokens"][4]
    prompts, limits = P + [P[0]], LIMITS + [0]
    res, stats = e.generate_queue(prompts, limits, stop_tokens=[stop], beams=3, return_stats=True, **KW)
    n_out = np.asarray([len(r[0]) for r in res])
    with e.queue_session(prompts, limits, stop_tokens=[stop], beams=3, device=device, **KW) as q:
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
                np.testing.assert_array_equal(tk[i, : count[i]], res[i][0])      # tokens, rows and score leave in that round
                np.testing.assert_array_equal(hd[i, : count[i]], res[i][1])
                assert sc[i] == np.float32(res[i][2]) or n_out[i] == 0
            prev_d = done
        again = q.advance()
        assert again[2] and np.array_equal(again[0], count)
        assert q.stats == stats and rounds > 2 and count.tolist() == n_out.tolist()
    after = e.generate_queue(prompts, limits, stop_tokens=[stop], beams=3, **KW)
    for a, b in zip(after, res):
        _equal(a, b)


def test_session_estate_and_end_midway(ctx73):
    e, P = ctx73.e, ctx73.prompts
    cfg = e.cfg
    L = _lib.load()
    ref = e.generate_queue(P, LIMITS, stop_tokens=[], beams=3, **KW)
    q = e.queue_session(P, LIMITS, stop_tokens=[], beams=3, **KW)
    count, done, finished = q.advance()
    assert not finished
    cat, rows, mx, toks, hid, n_out, sc = _raw_args(e, P[:2], [3, 3], 3)
    assert L.mi_gpt_queue_begin_beam(e._h, 2, cat.ctypes.data, _lib.i32p(rows), _lib.i32p(mx), None, 0, 0.7, 3, 3, toks.ctypes.data,
                                     hid.ctypes.data, 3, sc.ctypes.data, _lib.MI_HOST) == MI_ESTATE
    assert L.mi_gpt_generate_queue_beam(e._h, 2, cat.ctypes.data, _lib.i32p(rows), _lib.i32p(mx), None, 0, 0.7, 3, 3,
                                        toks.ctypes.data, hid.ctypes.data, 3, _lib.i32p(n_out), sc.ctypes.data, _lib.MI_HOST,
                                        None) == MI_ESTATE
    assert L.mi_gpt_queue_begin(e._h, 2, cat.ctypes.data, _lib.i32p(rows), _lib.i32p(mx), None, 0, 0.7, 3, toks.ctypes.data,
                                hid.ctypes.data, 3, _lib.MI_HOST, None, None, None, None) == MI_ESTATE
    assert L.mi_gpt_generate_beam(e._h, 2, cat.ctypes.data, _lib.i32p(rows), _lib.i32p(mx), None, 0, 0.7, 3, None, 3,
                                  toks.ctypes.data, hid.ctypes.data, 3, _lib.i32p(n_out), None, _lib.MI_HOST) == MI_ESTATE
    assert L.mi_gpt_generate_batch(e._h, 2, cat.ctypes.data, _lib.i32p(rows), _lib.i32p(mx), None, 0, 0.7, 3, None, toks.ctypes.data,
                                   hid.ctypes.data, 3, _lib.i32p(n_out), _lib.MI_HOST) == MI_ESTATE
    assert L.mi_gpt_reset(e._h) == MI_ESTATE
    assert b"session" in L.mi_last_error()
    count2, done2, _ = q.advance()                                   # the session went on undisturbed
    for i in np.nonzero(done2)[0]:
        np.testing.assert_array_equal(q.tokens[i, : count2[i]], ref[i][0])
        np.testing.assert_array_equal(q.hidden[i, : count2[i]], ref[i][1])
    q.end()                                                          # mid-way
    assert L.mi_gpt_queue_end(e._h) == MI_ESTATE
    res = e.generate_queue(P, LIMITS, stop_tokens=[], beams=3, **KW)
    for a, b in zip(res, ref):
        _equal(a, b)


def test_blocking_entry_on_device_arrays(ctx73):
    import torch
    e, P = ctx73.e, ctx73.prompts
    cfg = e.cfg
    ref = e.generate_queue(P, LIMITS, stop_tokens=[], beams=3, **KW)
    cat, rows, mx, toks, hid, n_out, sc = _raw_args(e, P, LIMITS, max(LIMITS))
    dev = torch.device("cuda", e.device)
    d_cat = torch.from_numpy(cat).to(dev)
    d_tok = torch.zeros(toks.shape, dtype=torch.int32, device=dev)
    d_hid = torch.zeros(hid.shape, dtype=torch.float32, device=dev)
    d_sc = torch.zeros(sc.shape, dtype=torch.float32, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    stats = np.zeros(2, np.int32)
    rc = _lib.load().mi_gpt_generate_queue_beam(e._h, 8, d_cat.data_ptr(), _lib.i32p(rows), _lib.i32p(mx), None, 0, 0.7, 3, 3,
                                                d_tok.data_ptr(), d_hid.data_ptr(), max(LIMITS), _lib.i32p(n_out), d_sc.data_ptr(),
                                                _lib.MI_DEVICE, stats.ctypes.data)
    assert rc == 0 and n_out.tolist() == LIMITS
    tk, hd, s = d_tok.cpu().numpy(), d_hid.cpu().numpy(), d_sc.cpu().numpy()
    for i in range(8):
        _equal((tk[i, : n_out[i]], hd[i, : n_out[i]], float(s[i])), ref[i])


def test_determinism_and_handle_hygiene(small, ctx73):
    e, P = ctx73.e, ctx73.prompts
    ones = np.ones((1, e.cfg.mel_codes), np.float32)
    sp = Sampling(1.0, 30, 0.8, 31)

    def others(e):
        g = e.generate_from_prompt(P[0], 12, stop_tokens=[], repeat_penality=ones, **KW)
        s = e.generate_from_prompt(P[0], 12, stop_tokens=[], repeat_penality=ones, sampling=sp, **KW)
        b, pen = e.generate_beam([P[0], P[2]], [12, 9], 3, stop_tokens=[], **KW)
        gq = e.generate_queue(P[:4], LIMITS[:4], stop_tokens=[], **KW)
        return g, s, b, pen, gq

    fresh = _engine(small, 7)                                         # a handle no queue-beam call has touched
    before = others(fresh)
    fresh.close()
    a, sa = e.generate_queue(P, LIMITS, stop_tokens=[], beams=3, return_stats=True, **KW)
    a2, sa2 = e.generate_queue(P, LIMITS, stop_tokens=[], beams=3, return_stats=True, **KW)      # the captured graphs by now
    _lib.prof_reset(); _lib.prof_enable(("attn",))                    # profiling: eager launches
    try:
        b, sb = e.generate_queue(P, LIMITS, stop_tokens=[], beams=3, return_stats=True, **KW)
    finally:
        _lib.prof_enable(())
    assert sa == sa2 == sb
    for i in range(8):
        _equal(a[i], a2[i])
        _equal(a[i], b[i])
    after = others(e)
    for x, y in ((before[0], after[0]), (before[1], after[1])):
        assert x[0].tolist() == y[0].tolist()
        np.testing.assert_array_equal(x[1], y[1])
    for x, y in zip(before[2], after[2]):
        _equal(x, y)
    np.testing.assert_array_equal(before[3], after[3])
    for x, y in zip(before[4], after[4]):
        assert x[0].tolist() == y[0].tolist()
        np.testing.assert_array_equal(x[1], y[1])


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_16_bit_engines(small, dtype):
    e = _engine(small, 7, dtype)
    P = [_prompt(e, 1 + b, TEXT[b]) for b in range(8)]
    res, stats = e.generate_queue(P, LIMITS, stop_tokens=[], beams=3, return_stats=True, **KW)
    assert [len(r[0]) for r in res] == LIMITS
    for toks, hid, score in res:
        assert toks.min() >= 0 and toks.max() < e.cfg.mel_codes
        assert np.isfinite(hid).all() and np.isfinite(score) and score < 0.0
    steps, passes = queue_schedule([p.shape[1] for p in P], LIMITS, LIMITS, 7, e.cfg.max_seq, beams=3)
    assert (stats["steps"], stats["passes"]) == (steps, len(passes))
    one = e.generate_queue(P, LIMITS, stop_tokens=[], beams=1, **KW)
    g = e.generate_queue(P, LIMITS, stop_tokens=[], **KW)
    for i in range(8):
        assert one[i][0].tolist() == g[i][0].tolist(), i
    e.close()
