"""GPU: IndexTTS GPT handles with more than 16 batch slots (max_batch up to 64): the wide matrix-core decode linear
(gemm_skinny_wide_kernel, 16-bit engines), the grouped fallback (fp32, a K that does not split), and everything that counts
slots — the batch, beam, sampled and queue entries, the packed prompt pass with more than 16 segments.

Shapes are those of test_generate_batch_template_widths / test_generate_batch_matrix_core_path (tests/test_gpu_gpt.py) with
max_batch raised.  Tolerances are the project's own bars for the same comparisons: fp32 against the engine's single-sentence path
2e-4 with identical tokens; f16 / bf16 against the oracle fed the engine's tokens 4e-2 / 2.5e-1 with the chosen logit within
6 tol of the maximum; beam scores against the same sentence alone bit for bit (tests/test_gpu_gpt_beam.py, _equal).  What the
engine promises beyond a tolerance is asserted exactly: a wide batch gives what its index-order groups of 16 give."""
import numpy as np
import pytest

from mi355tts import weights as W
from mi355tts import _lib
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


def _medium(hidden, heads, inner, max_batch):
    return IndexGPTConfig(hidden=hidden, layers=2, heads=heads, inner=inner, mel_codes=301, text_tokens=64, max_mel_pos=80,
                          max_text_pos=80, max_seq=96, max_batch=max_batch, start_mel_token=299, stop_mel_token=300)


def _small(max_batch, **kw):
    return IndexGPTConfig(**{**IndexGPTConfig.small().__dict__, "max_batch": max_batch, **kw})


def _groups(e, prompts, limits, cache=None, **kw):
    """generate_batch over index-order groups of 16 on the same handle -> (results, penalty rows); `cache` keeps a group's
    result by (first sentence, size): the groups of two batch sizes differ in the last one only"""
    res, pens = [], []
    for g in range(0, len(prompts), 16):
        key = (g, len(prompts[g:g + 16]))
        if cache is None or key not in cache:
            out = e.generate_batch(prompts[g:g + 16], limits[g:g + 16], **kw)
            if cache is None:
                cache = {}
            cache[key] = out
        r, p = cache[key]
        res += r
        pens.append(p)
    return res, np.concatenate(pens, 0)


# ---------------------------------------------------------------------------------------------------------------
# 1, 3, 7: fp32, 64 slots (the grouped fallback)
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide32():
    """One fp32 handle with 64 slots, 64 sentences of different lengths and limits, and each sentence decoded alone (computed
    once, left unchanged by the tests)."""
    cfg = _medium(256, 4, 1024, 64)
    st = W.synth_state(W.gpt_spec(cfg), 11)
    e = IndexGPT(cfg, st, dtype="f32")
    items = [_prompt(e, cfg, 10 + b, 3 + (b * 7) % 11, n_cond=8) for b in range(64)]
    limits = [6 + (b * 5) % 9 for b in range(64)]
    single = [e.generate_from_prompt(items[b][2], limits[b], stop_tokens=[], repeat_penality=_ones(cfg)) for b in range(64)]
    yield cfg, st, e, [it[2] for it in items], limits, single, {}
    e.close()


@pytest.mark.parametrize("nb", [17, 33, 40, 64])
def test_wide_batch_fp32_equals_single_and_groups(wide32, nb):
    cfg, st, e, prompts, limits, single, gcache = wide32
    res, pen = e.generate_batch(prompts[:nb], limits[:nb], stop_tokens=[])
    for b in range(nb):
        t, h, p = single[b]
        assert len(t) == limits[b] and res[b][0].tolist() == t.tolist(), b
        np.testing.assert_allclose(res[b][1], h, rtol=0, atol=2e-4)
        np.testing.assert_array_equal(pen[b:b + 1], p)
    # the fallback's definition: slots [16g, 16g + 16) run what they run as a batch of their own
    gres, gpen = _groups(e, prompts[:nb], limits[:nb], gcache, stop_tokens=[])
    for b in range(nb):
        np.testing.assert_array_equal(res[b][0], gres[b][0])
        np.testing.assert_array_equal(res[b][1], gres[b][1])
    np.testing.assert_array_equal(pen, gpen)


def test_bookkeeping_across_tiles(wide32):
    cfg, st, e, prompts, limits, single, _ = wide32
    nb = 40
    lim = list(limits[:nb])
    for b in (15, 16, 39):
        lim[b] = 0
    stop = int(single[20][0][2])                         # sentence 20 (limit 7) emits it as its third token at the latest
    res, pen = e.generate_batch(prompts[:nb], lim, stop_tokens=[stop])
    res2, pen2 = e.generate_batch(prompts[:nb], lim, stop_tokens=[stop])          # through the captured graph
    early = 0
    for b in range(nb):
        free = single[b][0].tolist()[: lim[b]]
        want = free[: free.index(stop) + 1] if stop in free else free
        assert res[b][0].tolist() == want, b
        assert res[b][1].shape == (len(want), cfg.hidden)
        early += b > 16 and len(want) < lim[b]
        np.testing.assert_array_equal(res2[b][0], res[b][0])
        np.testing.assert_array_equal(res2[b][1], res[b][1])
    np.testing.assert_array_equal(pen2, pen)
    assert [len(res[b][0]) for b in (15, 16, 39)] == [0, 0, 0]
    assert early >= 1 and len(res[20][0]) <= 3
    t, _, _ = e.generate_from_prompt(prompts[0], lim[0], stop_tokens=[stop], repeat_penality=_ones(cfg))
    assert t.tolist() == res[0][0].tolist()


def test_errors_and_hygiene(wide32):
    cfg, st, e, prompts, limits, single, _ = wide32
    with pytest.raises(_lib.MiError):
        IndexGPT(_medium(256, 4, 1024, 65), st, dtype="f32")
    # the C entry itself: NULL and a message
    L = _lib.load()
    blob = np.zeros(int(L.mi_gpt_param_count(_lib.i32p(np.asarray(cfg.to_int_array(), np.int32)), 10)), np.float32)
    ci = np.asarray(_medium(256, 4, 1024, 65).to_int_array(), np.int32)
    assert not L.mi_gpt_create(_lib.i32p(ci), len(ci), _lib.f32p(blob), blob.size, _lib.DTYPES["f32"], 0)
    assert b"max_batch" in L.mi_last_error()
    with pytest.raises(ValueError):
        e.generate_batch(prompts + prompts[:1], limits + limits[:1], stop_tokens=[])
    with pytest.raises(ValueError):
        e.generate_beam(prompts[:22], limits[:22], 3, stop_tokens=[])                 # 66 slots
    res, _ = e.generate_batch(prompts[:2], limits[:2], stop_tokens=[])                # still usable
    assert res[1][0].tolist() == single[1][0].tolist()
    # a 16-slot handle created afterwards: the tokens of test_generate_batch_template_widths[16]
    cfg16 = _medium(256, 4, 1024, 16)
    e16 = IndexGPT(cfg16, st, dtype="f32")
    res16, _ = e16.generate_batch(prompts[:16], limits[:16], stop_tokens=[])
    for b in range(16):
        assert res16[b][0].tolist() == single[b][0].tolist(), b
    e16.close()


# ---------------------------------------------------------------------------------------------------------------
# 2: 16-bit engines, the wide matrix-core kernel
# ---------------------------------------------------------------------------------------------------------------
def _teacher_forced_hidden(cfg, st, prompt, toks):
    """Oracle hidden states and logits when it is fed the ENGINE's tokens (16-bit engines may legitimately pick a different
    near-tie token than the fp32 oracle), from a penalty vector of ones that never changes (repeat_value = 1.0)."""
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


_ORACLE = {}


def _oracle(cfg, st, prompt, toks, b):
    key = (cfg.hidden, b, tuple(int(t) for t in toks))
    if key not in _ORACLE:
        _ORACLE[key] = _teacher_forced_hidden(cfg, st, prompt, toks)
    return _ORACLE[key]


@pytest.mark.parametrize("dtype,tol", [("f16", 4e-2), ("bf16", 2.5e-1)])
@pytest.mark.parametrize("nb", [19, 40, 64])
def test_wide_batch_matrix_core_path(dtype, tol, nb):
    """nb sentences on a 64-slot handle run the decode-step linears as ceil(nb / 16) column tiles per weight fragment where K
    splits (hidden 256: every layer, one 64-wide K block per wave and trip; hidden 320: inner 2560 takes the 8-way K split with
    five blocks per trip, K = 320 does not split and goes group by group).  Every index-order group of 16 has at least 3
    members, so with the threshold at 3 the groups run the 16-column kernel: (b) holds the wide kernel to it bit for bit."""
    saved = _lib.get_option("gpt_mfma_min")
    _lib.set_option("gpt_mfma_min", 3)
    try:
        for hidden, heads, inner in ((256, 4, 1024), (320, 5, 2560)):
            cfg = _medium(hidden, heads, inner, 64)
            st = W.synth_state(W.gpt_spec(cfg), 13)
            e = IndexGPT(cfg, st, dtype=dtype)
            items = [_prompt(e, cfg, 20 + b, 3 + (b * 5) % 9, n_cond=6) for b in range(nb)]
            prompts = [it[2] for it in items]
            limits = [5 + (b * 3) % 6 for b in range(nb)]
            res, _ = e.generate_batch(prompts, limits, stop_tokens=[], repeat_value=1.0)
            # (a) both sides of every column-tile boundary against the oracle
            for b in sorted({b for b in (0, 15, 16, 31, 32, nb - 1) if b < nb}):
                toks, hid = res[b]
                assert len(toks) == limits[b]
                ohid, ologits = _oracle(cfg, st, prompts[b], toks, b)
                np.testing.assert_allclose(hid, ohid, rtol=0, atol=tol)
                for k, t in enumerate(toks):
                    assert ologits[k, t] >= ologits[k].max() - 6 * tol, (b, k)
            # (b) slot independence
            gres, _ = _groups(e, prompts, limits, stop_tokens=[], repeat_value=1.0)
            for b in range(nb):
                np.testing.assert_array_equal(res[b][0], gres[b][0])
                np.testing.assert_array_equal(res[b][1], gres[b][1])
            e.close()
    finally:
        _lib.set_option("gpt_mfma_min", saved)


# ---------------------------------------------------------------------------------------------------------------
# 4: the queue with more than 16 slots
# ---------------------------------------------------------------------------------------------------------------
def test_queue_with_24_slots():
    cfg = _small(24, max_seq=640, max_mel_pos=640)
    st = W.synth_state(W.gpt_spec(cfg), SEED)
    e = IndexGPT(cfg, st, dtype="f32")
    n = 40
    prompts = [_prompt(e, cfg, 1 + b, 1 + b % 7)[2] for b in range(n)]              # 4 + (n_text + 2) + 1 <= 14 rows
    limits = [4 + (b * 5) % 13 for b in range(n)]
    assert max(p.shape[1] for p in prompts) <= 14
    res, stats = e.generate_queue(prompts, limits, stop_tokens=[], return_stats=True)
    for b in range(n):
        alone, _ = e.generate_batch([prompts[b]], [limits[b]], stop_tokens=[])
        assert len(res[b][0]) == limits[b] and res[b][0].tolist() == alone[0][0].tolist(), b
        np.testing.assert_allclose(res[b][1], alone[0][1], rtol=0, atol=2e-4)
    steps, passes = queue_schedule([p.shape[1] for p in prompts], limits, [len(t) for t, _ in res], 24, cfg.max_seq)
    assert (stats["steps"], stats["passes"]) == (steps, len(passes))
    assert len(passes[0]) == 24 and [s for _, s in passes[0]] == list(range(24))    # one packed pass of 24 segments
    e.close()


# ---------------------------------------------------------------------------------------------------------------
# 5: beams across the 16-slot line
# ---------------------------------------------------------------------------------------------------------------
def test_beams_across_the_16_slot_line():
    cfg = _small(24)
    st = W.synth_state(W.gpt_spec(cfg), SEED)
    e = IndexGPT(cfg, st, dtype="f32")
    kw = dict(repeat_value=0.7, penalty_range=3)
    prompts = [_prompt(e, cfg, 1 + b, 3 + b)[2] for b in range(7)]
    limits = [18 + (b * 5) % 7 for b in range(7)]
    both, pen = e.generate_beam(prompts, limits, 3, stop_tokens=[], **kw)           # 21 slots; group 5 = slots 15, 16, 17
    for g in range(7):
        alone, pa = e.generate_beam([prompts[g]], [limits[g]], 3, stop_tokens=[], **kw)
        assert len(alone[0][0]) == limits[g] and both[g][0].tolist() == alone[0][0].tolist(), g
        np.testing.assert_allclose(both[g][1], alone[0][1], rtol=0, atol=2e-4)
        np.testing.assert_array_equal(pen[g], pa[0])
        assert both[g][2] == alone[0][2], g                                         # the score, bit for bit
    e.close()


# ---------------------------------------------------------------------------------------------------------------
# 6: sampling
# ---------------------------------------------------------------------------------------------------------------
def test_sampling_with_20_slots():
    cfg = _small(20)
    st = W.synth_state(W.gpt_spec(cfg), SEED)
    e = IndexGPT(cfg, st, dtype="f32")
    s = 100
    prompts = [_prompt(e, cfg, 1 + b, 1 + b % 9)[2] for b in range(20)]
    limits = [10 + (b * 3) % 8 for b in range(20)]
    sp = [Sampling(1.0, 30, 0.8, s + b) for b in range(20)]
    res, pen = e.generate_batch(prompts, limits, stop_tokens=[], sampling=sp)
    for b in range(20):
        t, h, p = e.generate_from_prompt(prompts[b], limits[b], stop_tokens=[], repeat_penality=_ones(cfg), sampling=sp[b])
        assert len(t) == limits[b] and res[b][0].tolist() == t.tolist(), b
        np.testing.assert_array_equal(pen[b:b + 1], p)
    # the same seed and prompt in slots 3 and 18: the same take
    prompts[18], limits[18], sp[18] = prompts[3], limits[3], sp[3]
    res2, _ = e.generate_batch(prompts, limits, stop_tokens=[], sampling=sp)
    assert res2[18][0].tolist() == res2[3][0].tolist() == res[3][0].tolist()
    np.testing.assert_array_equal(res2[18][1], res2[3][1])
    e.close()


# ---------------------------------------------------------------------------------------------------------------
# 8: full size, once
# ---------------------------------------------------------------------------------------------------------------
def test_full_size_40_slots():
    """IndexTTS-1.5 size in f16, three column tiles at the real layer shapes (K = 1280: four-way K split, K = 5120: eight-way,
    five blocks per trip).  The same prompt in all 40 slots: every slot decodes slot 0's tokens and rows bit for bit, and slot 0's
    first tokens hold the teacher-forced bar of test_full_size_gpt_teacher_forced_and_batch_equals_single."""
    cfg = IndexGPTConfig()
    assert (cfg.layers, cfg.hidden, cfg.heads) == (24, 1280, 20)
    cfg.max_batch = 40
    st = W.synth_state(W.gpt_spec(cfg), SEED, fast=True)
    e = IndexGPT(cfg, st, dtype="f16")
    _, _, p = _prompt(e, cfg, 3, 12, n_cond=32)
    n_new = 12
    res, _ = e.generate_batch([p] * 40, [n_new] * 40, stop_tokens=[])
    assert len(res[0][0]) == n_new and np.isfinite(res[0][1]).all()
    for b in range(1, 40):
        np.testing.assert_array_equal(res[b][0], res[0][0])
        np.testing.assert_array_equal(res[b][1], res[0][1])
    n_chk = 4
    oh, _ = _teacher_forced_hidden(cfg, st, p, res[0][0][:n_chk])
    assert float(np.abs(oh).max()) > 0.1
    assert float(np.abs(res[0][1][:n_chk] - oh).max()) < 4e-2 * max(1.0, float(np.abs(oh).max()))
    e.close()
