"""GPU: the sentence queue as a session (mi_gpt_queue_begin / _advance / _end; IndexGPT.queue_session): the loop of
mi_gpt_generate_queue handed back after every run of decode steps, with the rows a round produced copied out by one kernel
(csrc/gpt_prompt.hip gpt_copy_out_kernel).  The blocking entry runs the same loop, so everything is held to it with
assert_array_equal: tokens, rows, counts and stats; and every prefix a round hands out is already the final one, bit for bit.

The fixture restates that of tests/test_gpu_gpt_queue.py: IndexGPTConfig.small() with three slots, fp32, eight sentences."""
import numpy as np
import pytest

from mi355tts import weights as W
from mi355tts import _lib
from mi355tts.config import IndexGPTConfig
from mi355tts.indextts import IndexGPT, Sampling
from oracle import gpt_np as O

pytestmark = pytest.mark.gpu
SEED = 9527
MI_ESTATE = -4                             # include/mi355tts.h


def _prompt(e, cfg, seed, n_text, n_cond=4):
    conds = W.synth_normal(seed, "conds", (1, n_cond, cfg.hidden), std=0.5)
    text = (np.arange(n_text, dtype=np.int32) * 5 + seed) % (cfg.text_tokens - 2) + 2
    mh, _ = e.mel_embed(cfg.start_mel_token, 0)
    p, _ = e.concat(conds, e.text_embed(text), mh)
    return conds, text, p


@pytest.fixture(scope="module")
def small3():
    cfg = IndexGPTConfig(**{**IndexGPTConfig.small().__dict__, "max_batch": 3})
    st = W.synth_state(W.gpt_spec(cfg), SEED)
    e = IndexGPT(cfg, st, dtype="f32")
    items = [_prompt(e, cfg, 1 + b, (6, 3, 9, 5, 1, 8, 4, 7)[b]) for b in range(8)]
    limits = [14, 9, 11, 3, 12, 1, 10, 6]
    o_free, _, _ = O.generate(cfg, st, items[1][0], items[1][1], max_generate_length=items[1][2].shape[1] + 9, stop_tokens=[])
    stop = o_free[4]                       # ends sentence 1 early
    yield cfg, e, [it[2] for it in items], limits, stop
    e.close()


def _host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def _drive(e, prompts, limits, *, device, **kw):
    """a session to its end; at every round: counts and done flags never go back, finished comes exactly when all are done, and
    the prefixes handed out are kept for the comparison with the final arrays"""
    n = len(prompts)
    snaps = []
    with e.queue_session(prompts, limits, device=device, **kw) as q:
        prev_c, prev_d = np.zeros(n, np.int32), np.zeros(n, bool)
        finished, rounds = False, 0
        while not finished:
            count, done, finished = q.advance()
            rounds += 1
            assert rounds < 200
            assert np.all(count >= prev_c) and np.all(done >= prev_d)
            assert np.all(count[prev_d] == prev_c[prev_d])           # a finished sentence does not grow
            assert np.all(count <= np.asarray(limits))
            assert finished == bool(np.all(done))
            snaps.append((count, _host(q.tokens).copy(), _host(q.hidden).copy()))
            prev_c, prev_d = count, done
        again = q.advance()                                          # after the end: nothing happens, the same report
        assert again[2] and np.array_equal(again[0], count) and np.array_equal(again[1], done)
        tokens, hidden, stats = _host(q.tokens).copy(), _host(q.hidden).copy(), q.stats
    for count, tk, hd in snaps:
        for i in range(n):
            np.testing.assert_array_equal(tk[i, : count[i]], tokens[i, : count[i]])
            np.testing.assert_array_equal(hd[i, : count[i]], hidden[i, : count[i]])
    return prev_c, tokens, hidden, stats, rounds


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_session_equals_generate_queue(small3, device, sampled):
    cfg, e, prompts, limits, stop = small3
    prompts, limits = prompts + [prompts[0]], limits + [0]           # ... and a sentence with max_new = 0
    kw = {"stop_tokens": [stop]}
    if sampled:
        kw["sampling"] = [Sampling(0.9, 20, 0.9, 1000 + i) if i != 2 else None for i in range(len(prompts))]
    res, stats = e.generate_queue(prompts, limits, return_stats=True, **kw)
    count, tokens, hidden, sstats, rounds = _drive(e, prompts, limits, device=device, **kw)
    assert count.tolist() == [len(t) for t, _ in res] and count[-1] == 0
    if not sampled:
        assert count[1] < limits[1] and tokens[1, count[1] - 1] == stop
    for i, (t, h) in enumerate(res):
        np.testing.assert_array_equal(tokens[i, : count[i]], t)
        np.testing.assert_array_equal(hidden[i, : count[i]], h)
    assert sstats == stats and rounds > 2
    # the handle is as usable as before
    res2 = e.generate_queue(prompts, limits, **kw)
    for (t, h), (t2, h2) in zip(res, res2):
        np.testing.assert_array_equal(t, t2)
        np.testing.assert_array_equal(h, h2)


def test_other_entries_return_estate_and_end_midway(small3):
    cfg, e, prompts, limits, stop = small3
    L = _lib.load()
    ref = e.generate_queue(prompts, limits, stop_tokens=[stop])
    q = e.queue_session(prompts, limits, stop_tokens=[stop])
    count, done, finished = q.advance()
    assert not finished and count.sum() > 0
    rows = np.ascontiguousarray([p.shape[1] for p in prompts[:2]], np.int32)
    cat = np.ascontiguousarray(np.concatenate([p.reshape(-1, cfg.hidden) for p in prompts[:2]]))
    mx = np.asarray([3, 3], np.int32)
    toks, hid = np.zeros((2, 3), np.int32), np.zeros((2, 3, cfg.hidden), np.float32)
    n_out = np.zeros(2, np.int32)
    # a second begin
    assert L.mi_gpt_queue_begin(e._h, 2, cat.ctypes.data, _lib.i32p(rows), _lib.i32p(mx), None, 0, 1.0, 8, toks.ctypes.data,
                                hid.ctypes.data, 3, _lib.MI_HOST, None, None, None, None) == MI_ESTATE
    # generate_batch
    assert L.mi_gpt_generate_batch(e._h, 2, cat.ctypes.data, _lib.i32p(rows), _lib.i32p(mx), None, 0, 1.0, 8, None, toks.ctypes.data,
                                   hid.ctypes.data, 3, _lib.i32p(n_out), _lib.MI_HOST) == MI_ESTATE
    # step
    last, tok, logits = np.zeros(cfg.hidden, np.float32), np.zeros(1, np.int32), np.zeros(cfg.mel_codes, np.float32)
    assert L.mi_gpt_step(e._h, cat.ctypes.data, 1, None, 1, last.ctypes.data, tok.ctypes.data, logits.ctypes.data,
                         _lib.MI_HOST) == MI_ESTATE
    assert L.mi_gpt_reset(e._h) == MI_ESTATE
    assert b"session" in L.mi_last_error()
    with pytest.raises(_lib.MiError):
        e.generate_queue(prompts, limits, stop_tokens=[stop])
    # the session went on undisturbed: its next round still hands out final prefixes
    count2, _, _ = q.advance()
    for i in range(len(prompts)):
        np.testing.assert_array_equal(q.tokens[i, : count2[i]], ref[i][0][: count2[i]])
        np.testing.assert_array_equal(q.hidden[i, : count2[i]], ref[i][1][: count2[i]])
    q.end()                                                          # mid-way
    assert L.mi_gpt_queue_end(e._h) == MI_ESTATE                      # nothing is open any more
    cnt = np.zeros(8, np.int32)
    assert L.mi_gpt_queue_advance(e._h, cnt.ctypes.data, cnt.ctypes.data, cnt.ctypes.data, None) == MI_ESTATE
    res = e.generate_queue(prompts, limits, stop_tokens=[stop])
    for (t, h), (t2, h2) in zip(ref, res):
        np.testing.assert_array_equal(t, t2)
        np.testing.assert_array_equal(h, h2)
    # validation is generate_queue's, before anything is launched, and leaves no session behind
    with pytest.raises(ValueError):
        e.queue_session(prompts, [cfg.max_mel_pos + 1] + limits[1:], stop_tokens=[stop])
    assert e.generate_queue(prompts[:1], [2], stop_tokens=[])[0][0].size == 2


def test_destroy_with_an_open_session(small3):
    cfg, _, prompts, limits, stop = small3
    e = IndexGPT(cfg, W.synth_state(W.gpt_spec(cfg), SEED), dtype="f32")
    q = e.queue_session(prompts, limits, stop_tokens=[stop])
    q.advance()
    e.close()
    q.end()                                                          # the handle is gone: nothing to do, no error


def test_schedule_through_the_session():
    """the two-slot case of test_gpu_gpt_queue.py::test_schedule_is_real: limits (65, 17, 17, 17, 17) take 64 decode steps in 4
    passes through the session as well"""
    cfg = IndexGPTConfig(hidden=256, layers=2, heads=4, inner=1024, mel_codes=301, text_tokens=64, max_mel_pos=80,
                         max_text_pos=80, max_seq=96, max_batch=2, start_mel_token=299, stop_mel_token=300)
    st = W.synth_state(W.gpt_spec(cfg), 11)
    e = IndexGPT(cfg, st, dtype="f32")
    try:
        prompts = [_prompt(e, cfg, 10 + b, 3 + (b * 7) % 11, n_cond=8)[2] for b in range(5)]
        limits = [65, 17, 17, 17, 17]
        res, stats = e.generate_queue(prompts, limits, stop_tokens=[], return_stats=True)
        count, tokens, hidden, sstats, _ = _drive(e, prompts, limits, device=False, stop_tokens=[])
        assert count.tolist() == limits
        assert (sstats["steps"], sstats["passes"]) == (64, 4) and sstats == stats
        for i, (t, h) in enumerate(res):
            np.testing.assert_array_equal(tokens[i, : count[i]], t)
            np.testing.assert_array_equal(hidden[i, : count[i]], h)
    finally:
        e.close()
