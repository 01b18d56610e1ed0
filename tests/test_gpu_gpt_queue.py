"""GPU: the sentence queue of the IndexTTS GPT (mi_gpt_generate_queue / IndexGPT.generate_queue): any number of sentences
through the handle's slots, a slot refilled as soon as its sentence stops, the prompts admitted together run as one packed
pass (csrc/gpt_prompt.hip).

Tolerances are the project's own (tests/test_gpu_gpt.py): fp32 against the numpy oracle 3e-4, fp32 against the engine's
single-sentence path 2e-4 (the packed pass differs from it in GEMM tiling, i.e. summation order, only), f16 / bf16 against the
oracle fed the engine's tokens 4e-2 / 2.5e-1 with the chosen logit within 6 tol of the maximum.  The entry's stats are held
against the host model of the stated policy (queue_schedule), evaluated on the lengths the engine produced."""
import numpy as np
import pytest

from mi355tts import weights as W
from mi355tts import _lib
from mi355tts import indextts as IX
from mi355tts.config import IndexGPTConfig
from mi355tts.indextts import IndexGPT, Sampling, queue_schedule
from oracle import gpt_np as O

pytestmark = pytest.mark.gpu
SEED = 9527


def _prompt(e, cfg, seed, n_text, n_cond=4):
    conds = W.synth_normal(seed, "conds", (1, n_cond, cfg.hidden), std=0.5)
    text = (np.arange(n_text, dtype=np.int32) * 5 + seed) % (cfg.text_tokens - 2) + 2
    mh, _ = e.mel_embed(cfg.start_mel_token, 0)
    p, _ = e.concat(conds, e.text_embed(text), mh)
    return conds, text, p


def _ones(cfg):
    return np.ones((1, cfg.mel_codes), np.float32)


def _model(cfg, prompts, limits, res):
    steps, passes = queue_schedule([p.shape[1] for p in prompts], limits, [len(t) for t, _ in res], cfg.max_batch, cfg.max_seq)
    return steps, passes


def _teacher_forced_hidden(cfg, st, prompt, toks):
    """Oracle hidden states and logits when it is fed the ENGINE's tokens, from a penalty vector of ones that never changes
    (the callers decode with repeat_value = 1.0)."""
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


@pytest.fixture(scope="module")
def small3():
    """IndexGPTConfig.small() with three slots, fp32, and eight sentences of different text lengths and limits."""
    cfg = IndexGPTConfig(**{**IndexGPTConfig.small().__dict__, "max_batch": 3})
    st = W.synth_state(W.gpt_spec(cfg), SEED)
    e = IndexGPT(cfg, st, dtype="f32")
    items = [_prompt(e, cfg, 1 + b, (6, 3, 9, 5, 1, 8, 4, 7)[b]) for b in range(8)]
    limits = [14, 9, 11, 3, 12, 1, 10, 6]
    yield cfg, st, e, items, limits
    e.close()


@pytest.fixture(scope="module")
def small3_run(small3):
    """One queue run shared by the tests below (left unchanged by them): a stop id the oracle emits early in sentence 1."""
    cfg, st, e, items, limits = small3
    o_free, _, _ = O.generate(cfg, st, items[1][0], items[1][1], max_generate_length=items[1][2].shape[1] + 9, stop_tokens=[])
    stop = o_free[4]
    res, stats = e.generate_queue([it[2] for it in items], limits, stop_tokens=[stop], return_stats=True)
    return stop, res, stats


def test_queue_fp32_against_the_oracle_and_the_single_path(small3, small3_run):
    cfg, st, e, items, limits = small3
    stop, res, stats = small3_run
    assert len(res) == 8
    for b, (conds, text, p) in enumerate(items):
        ot, oh, _ = O.generate(cfg, st, conds, text, max_generate_length=p.shape[1] + limits[b], stop_tokens=[stop])
        assert res[b][0].tolist() == ot, b
        np.testing.assert_allclose(res[b][1], oh, rtol=0, atol=3e-4)
        t, h, _ = e.generate_from_prompt(p, limits[b], stop_tokens=[stop], repeat_penality=_ones(cfg))
        assert res[b][0].tolist() == t.tolist(), b
        np.testing.assert_allclose(res[b][1], h, rtol=0, atol=2e-4)
    assert len(res[1][0]) <= 5 and res[1][0][-1] == stop
    # the schedule the entry ran is the stated policy's, on the lengths it produced
    steps, passes = _model(cfg, [it[2] for it in items], limits, res)
    assert (stats["steps"], stats["passes"]) == (steps, len(passes))
    assert len(passes) > 1


def test_schedule_is_real():
    """Two slots, limits [65, 17, 17, 17, 17], no stop ids: 64 decode steps in 4 passes (index-order groups of two need 96)."""
    cfg = IndexGPTConfig(hidden=256, layers=2, heads=4, inner=1024, mel_codes=301, text_tokens=64, max_mel_pos=80,
                         max_text_pos=80, max_seq=96, max_batch=2, start_mel_token=299, stop_mel_token=300)
    st = W.synth_state(W.gpt_spec(cfg), 11)
    e = IndexGPT(cfg, st, dtype="f32")
    items = [_prompt(e, cfg, 10 + b, 3 + (b * 7) % 11, n_cond=8) for b in range(5)]
    limits = [65, 17, 17, 17, 17]
    prompts = [it[2] for it in items]
    res, stats = e.generate_queue(prompts, limits, stop_tokens=[], return_stats=True)
    assert [len(t) for t, _ in res] == limits
    assert (stats["steps"], stats["passes"]) == (64, 4)
    steps, passes = _model(cfg, prompts, limits, res)
    assert (steps, len(passes)) == (64, 4)
    for b in (0, 4):
        t, h, _ = e.generate_from_prompt(prompts[b], limits[b], stop_tokens=[], repeat_penality=_ones(cfg))
        assert res[b][0].tolist() == t.tolist(), b
        np.testing.assert_allclose(res[b][1], h, rtol=0, atol=2e-4)
    e.close()


def test_edges(small3):
    cfg, st, e, items, limits = small3
    prompts = [it[2] for it in items]
    # n <= max_batch: the tokens of generate_batch
    bres, _ = e.generate_batch(prompts[:3], limits[:3], stop_tokens=[])
    qres = e.generate_queue(prompts[:3], limits[:3], stop_tokens=[])
    for b in range(3):
        assert qres[b][0].tolist() == bres[b][0].tolist(), b
        np.testing.assert_allclose(qres[b][1], bres[b][1], rtol=0, atol=2e-4)
    # n = 1
    one, stats = e.generate_queue(prompts[2:3], [7], stop_tokens=[], return_stats=True)
    assert one[0][0].tolist() == bres[2][0][:7].tolist() and stats == {"steps": 6, "passes": 1}
    # max_new of 0 and of 1: no slot and n_out = 0; one token right after the prompt pass
    res, stats = e.generate_queue(prompts[:4], [0, 1, 5, 0], stop_tokens=[], return_stats=True)
    assert [len(t) for t, _ in res] == [0, 1, 5, 0] and res[0][1].shape == (0, cfg.hidden)
    assert res[1][0].tolist() == bres[1][0][:1].tolist() and res[2][0].tolist() == bres[2][0][:5].tolist()
    assert stats == {"steps": 4, "passes": 1}
    res, stats = e.generate_queue(prompts[:2], [0, 0], stop_tokens=[], return_stats=True)
    assert [len(t) for t, _ in res] == [0, 0] and stats == {"steps": 0, "passes": 0}
    # a sentence whose token 0 is the stop id: it retires after its prompt pass and the next one takes its slot at once
    stop0 = int(bres[1][0][0])
    four = [prompts[0], prompts[1], prompts[2], prompts[0]]
    res, stats = e.generate_queue(four, [6, 6, 6, 6], stop_tokens=[stop0], return_stats=True)
    assert res[1][0].tolist() == [stop0] and res[3][0].tolist() == res[0][0].tolist()
    for b in (0, 2):
        t, _, _ = e.generate_from_prompt(four[b], 6, stop_tokens=[stop0], repeat_penality=_ones(cfg))
        assert res[b][0].tolist() == t.tolist(), b
    steps, passes = queue_schedule([p.shape[1] for p in four], [6] * 4, [len(t) for t, _ in res], cfg.max_batch, cfg.max_seq)
    assert passes[0] == [(0, 0), (1, 1), (2, 2)] and len(passes) == 2 and passes[1][0][0] == 3
    assert (stats["steps"], stats["passes"]) == (steps, 2)
    # a one-row prompt alone in its pass (the single-row path), and packed with another prompt
    mh, _ = e.mel_embed(cfg.start_mel_token, 0)
    t1, h1, _ = e.generate_from_prompt(mh, 5, stop_tokens=[], repeat_penality=_ones(cfg))
    res = e.generate_queue([mh], [5], stop_tokens=[])
    assert res[0][0].tolist() == t1.tolist()
    np.testing.assert_allclose(res[0][1], h1, rtol=0, atol=2e-4)
    res = e.generate_queue([prompts[0], mh], [4, 5], stop_tokens=[])
    assert res[1][0].tolist() == t1.tolist() and res[0][0].tolist() == bres[0][0][:4].tolist()
    np.testing.assert_allclose(res[1][1], h1, rtol=0, atol=2e-4)


def test_packed_attention_long_prompts():
    """A 530-row prompt packed with a 7-row one (more than 512 keys through the kernel's strided key loop, the short segment
    behind the long one), then two prompts that do not fit one pass together.  Against the oracle's prompt pass and steps."""
    cfg = IndexGPTConfig(**{**IndexGPTConfig.small().__dict__, "max_seq": 640, "max_mel_pos": 640, "max_batch": 2})
    st = W.synth_state(W.gpt_spec(cfg), 3)
    e = IndexGPT(cfg, st, dtype="f32")
    pa = W.synth_normal(9, "pa", (1, 530, cfg.hidden), std=0.7)
    pb = W.synth_normal(9, "pb", (1, 7, cfg.hidden), std=0.7)
    pc = W.synth_normal(9, "pc", (1, 200, cfg.hidden), std=0.7)
    ref = {}
    for name, p in (("a", pa), ("b", pb), ("c", pc)):
        res1 = e.generate_from_prompt(p, 3, stop_tokens=[], repeat_value=1.0, repeat_penality=_ones(cfg))
        ref[name] = (res1[0],) + _teacher_forced_hidden(cfg, st, p, res1[0])

    def check(res, names):
        for (toks, hid), name in zip(res, names):
            t1, ohid, ologits = ref[name]
            assert toks.tolist() == t1.tolist() and len(toks) == 3, name
            np.testing.assert_allclose(hid, ohid, rtol=0, atol=3e-4)
            assert toks.tolist() == [int(np.argmax(ologits[k])) for k in range(3)], name

    for prompts, names in (([pa, pb], "ab"), ([pb, pa], "ba")):
        res, stats = e.generate_queue(prompts, [3, 3], stop_tokens=[], repeat_value=1.0, return_stats=True)
        assert stats == {"steps": 2, "passes": 1}
        check(res, names)
    res, stats = e.generate_queue([pa, pc, pb], [3, 3, 3], stop_tokens=[], repeat_value=1.0, return_stats=True)
    assert stats["passes"] == 3          # 530 + 200 rows exceed the 640-row scratch: pass 2 is the 200-row prompt alone
    assert queue_schedule([530, 200, 7], [3] * 3, [3] * 3, 2, 640) == (stats["steps"], [[(0, 0)], [(1, 1)], [(2, 0)]])
    check(res, "acb")
    e.close()


def test_slot_reuse_reads_nothing_stale(small3):
    """Two of the three slots aside: with max_batch = 2 a long sentence (16-row prompt, 12 tokens) is followed in the same slot
    by a short one (8-row prompt): cache rows, penalty entries and tokens of the first are still there and must not be read."""
    cfg0, st, _, _, _ = small3
    cfg = IndexGPTConfig(**{**cfg0.__dict__, "max_batch": 2})
    e = IndexGPT(cfg, st, dtype="f32")
    a, b, c = _prompt(e, cfg, 3, 9)[2], _prompt(e, cfg, 6, 8)[2], _prompt(e, cfg, 5, 1)[2]
    limits = [12, 30, 9]
    res, stats = e.generate_queue([a, b, c], limits, stop_tokens=[], return_stats=True)
    steps, passes = queue_schedule([p.shape[1] for p in (a, b, c)], limits, limits, 2, cfg.max_seq)
    assert passes == [[(0, 0), (1, 1)], [(2, 0)]] and (stats["steps"], stats["passes"]) == (steps, 2)
    for p, lim, (toks, hid) in zip((a, b, c), limits, res):
        t, h, _ = e.generate_from_prompt(p, lim, stop_tokens=[], repeat_penality=_ones(cfg))
        assert toks.tolist() == t.tolist()
        np.testing.assert_allclose(hid, h, rtol=0, atol=2e-4)
    e.close()


@pytest.mark.parametrize("dtype,tol", [("f16", 4e-2), ("bf16", 2.5e-1)])
def test_queue_16bit_matrix_core_steps(dtype, tol):
    """16 slots, 20 sentences; the decode steps run as MFMA skinny GEMMs (threshold lowered to 3 as in test_gpu_gpt.py); 16
    prompts of up to 20 rows do not fit the 96-row scratch, so the admission splits by capacity."""
    saved = _lib.get_option("gpt_mfma_min")
    _lib.set_option("gpt_mfma_min", 3)
    try:
        cfg = IndexGPTConfig(hidden=256, layers=2, heads=4, inner=1024, mel_codes=301, text_tokens=64, max_mel_pos=80,
                             max_text_pos=80, max_seq=96, max_batch=16, start_mel_token=299, stop_mel_token=300)
        st = W.synth_state(W.gpt_spec(cfg), 13)
        e = IndexGPT(cfg, st, dtype=dtype)
        items = [_prompt(e, cfg, 20 + b, 3 + (b * 5) % 9, n_cond=6) for b in range(20)]
        limits = [5 + (b * 3) % 6 for b in range(20)]
        prompts = [it[2] for it in items]
        res, stats = e.generate_queue(prompts, limits, stop_tokens=[], repeat_value=1.0, return_stats=True)
        assert [len(t) for t, _ in res] == limits
        steps, passes = _model(cfg, prompts, limits, res)
        assert (stats["steps"], stats["passes"]) == (steps, len(passes)) and len(passes) >= 3
        for b in (0, 9, 19):
            toks, hid = res[b]
            ohid, ologits = _teacher_forced_hidden(cfg, st, prompts[b], toks)
            np.testing.assert_allclose(hid, ohid, rtol=0, atol=tol)
            for k, t in enumerate(toks):
                assert ologits[k, t] >= ologits[k].max() - 6 * tol, (b, k)
        e.close()
    finally:
        _lib.set_option("gpt_mfma_min", saved)


def test_queue_sampling_equals_the_single_path(small3):
    """Per-sentence Sampling and None mixed: a sentence's draws depend on its seed and decode index alone, so the tokens are
    generate_from_prompt's (the two paths' logits differ by the prompt pass's rounding only)."""
    cfg, st, e, items, limits = small3
    prompts = [it[2] for it in items[:6]]
    lim = [10, 9, 11, 3, 12, 7]
    samp = [Sampling(0.9, 8, 0.9, seed=101), None, Sampling(1.0, 0, 0.8, seed=7), Sampling(1.3, 5, 1.0, seed=2 ** 40 + 3), None,
            Sampling(0.7, 30, 0.6, seed=55)]
    res = e.generate_queue(prompts, lim, stop_tokens=[], sampling=samp)
    greedy = e.generate_queue(prompts, lim, stop_tokens=[])
    for b in range(6):
        t, h, _ = e.generate_from_prompt(prompts[b], lim[b], stop_tokens=[], repeat_penality=_ones(cfg), sampling=samp[b])
        assert res[b][0].tolist() == t.tolist(), b
        np.testing.assert_allclose(res[b][1], h, rtol=0, atol=2e-4)
        if samp[b] is None:
            assert res[b][0].tolist() == greedy[b][0].tolist()
    assert any(res[b][0].tolist() != greedy[b][0].tolist() for b in (0, 2, 3, 5))      # the draws are real
    # one Sampling for all, and a list of the wrong length
    res1 = e.generate_queue(prompts[:2], lim[:2], stop_tokens=[], sampling=samp[0])
    assert res1[0][0].tolist() == res[0][0].tolist()
    with pytest.raises(ValueError):
        e.generate_queue(prompts, lim, sampling=samp[:3])


def test_handle_hygiene_and_errors(small3, small3_run):
    cfg, st, e, items, limits = small3
    stop, res, stats = small3_run
    prompts = [it[2] for it in items]
    bres, bpen = e.generate_batch(prompts[:3], limits[:3], stop_tokens=[stop])
    t0, h0, _ = e.generate_from_prompt(prompts[0], limits[0], stop_tokens=[stop], repeat_penality=_ones(cfg))
    # twice: identical output (the second call replays the captured decode step)
    res2, stats2 = e.generate_queue(prompts, limits, stop_tokens=[stop], return_stats=True)
    assert stats2 == stats
    for b in range(8):
        assert res2[b][0].tolist() == res[b][0].tolist()
        np.testing.assert_array_equal(res2[b][1], res[b][1])

    def still_fine():
        r, pen = e.generate_batch(prompts[:3], limits[:3], stop_tokens=[stop])
        for b in range(3):
            assert r[b][0].tolist() == bres[b][0].tolist()
            np.testing.assert_array_equal(r[b][1], bres[b][1])
        np.testing.assert_array_equal(pen, bpen)
        t, h, _ = e.generate_from_prompt(prompts[0], limits[0], stop_tokens=[stop], repeat_penality=_ones(cfg))
        assert t.tolist() == t0.tolist()
        np.testing.assert_array_equal(h, h0)
        q = e.generate_queue(prompts[:4], limits[:4], stop_tokens=[stop])
        for b in range(4):
            assert q[b][0].tolist() == res[b][0].tolist()

    still_fine()
    # a sentence with prompt_rows + max_new - 1 > max_seq
    longp = _prompt(e, cfg, 9, 22)[2]
    assert longp.shape[1] == 29 and 37 <= cfg.max_mel_pos and 29 + 37 - 1 == cfg.max_seq + 1
    with pytest.raises(ValueError):
        e.generate_queue([prompts[0], prompts[1], longp, prompts[3]], [3, 3, 37, 3], stop_tokens=[])
    # max_new > cap, and a half-given set of sampling arrays, at the C-ABI (the wrapper always sizes cap and gives all four)
    ps = [np.ascontiguousarray(p, dtype=np.float32).reshape(-1, cfg.hidden) for p in prompts[:2]]
    cat = np.ascontiguousarray(np.concatenate(ps, axis=0))
    rows = np.ascontiguousarray([p.shape[0] for p in ps], dtype=np.int32)
    mx = np.ascontiguousarray([4, 6], dtype=np.int32)
    stops = np.zeros((0,), np.int32)
    with pytest.raises(ValueError):
        IX._queue_call(e._h, cfg, cat, rows, mx, stops, 0.7, 10, 5, None)
    T, K, Pp, Sd = IX._sampling_arrays([Sampling(seed=1), Sampling(seed=2)])
    with pytest.raises(ValueError):
        IX._queue_call(e._h, cfg, cat, rows, mx, stops, 0.7, 10, 6, (T, K, None, Sd))
    with pytest.raises(ValueError):
        IX._queue_call(e._h, cfg, cat, rows, mx, stops, 0.7, 10, 6, (T, K, Pp, None))
    with pytest.raises(ValueError):
        e.generate_queue([], [])
    still_fine()


def test_full_size_queue():
    """IndexTTS-1.5 size (24 x 1280, f16): 6 sentences through 4 slots.  16-bit rounding differs between the packed pass / batched
    step and the single-sentence kernels, so, as in the existing full-size test, tokens must agree with the single path on at
    least the first half of each sentence; the schedule is the model's."""
    cfg = IndexGPTConfig()
    assert (cfg.layers, cfg.hidden, cfg.heads) == (24, 1280, 20)
    cfg.max_batch = 4
    st = W.synth_state(W.gpt_spec(cfg), SEED, fast=True)
    e = IndexGPT(cfg, st, dtype="f16")
    prompts = [_prompt(e, cfg, 3 + b, 12 - b, n_cond=32)[2] for b in range(6)]
    limits = [12, 5, 9, 12, 7, 10]
    res, stats = e.generate_queue(prompts, limits, stop_tokens=[], return_stats=True)
    assert [len(t) for t, _ in res] == limits
    steps, passes = _model(cfg, prompts, limits, res)
    assert (stats["steps"], stats["passes"]) == (steps, len(passes)) and len(passes) >= 2
    for b in range(6):
        t, h, _ = e.generate_from_prompt(prompts[b], limits[b], stop_tokens=[], repeat_penality=_ones(cfg))
        assert np.isfinite(res[b][1]).all()
        k = 0
        while k < limits[b] and res[b][0][k] == t[k]:
            k += 1
        assert k >= (limits[b] + 1) // 2, (b, k)
    e.close()
