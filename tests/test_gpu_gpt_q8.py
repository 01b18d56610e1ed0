"""GPU: IndexTTS GPT handles with per-channel uint8 weights (IndexGPT(..., weights="q8"), mi_gpt_create_q8; csrc/gpt_q8.hip).

A q8 handle's weights are worth the dequantised blob weights.gpt_q8_dequantized_blob, so every comparison is against that:
  * an f16 handle built from the dequantised blob stores f16(float32(q - zp) * scale) — exactly what the q8 handle's prompt passes
    read from the dequantise kernel's scratch — so prompt passes of two or more rows agree bit for bit (E1);
  * the oracle (oracle/gpt_np.py, unchanged) on gpt_q8_ref.dequantized_state, fed the engine's tokens, with the project's bar for
    16-bit engines: hidden rows within 4e-2, the chosen logit within 6 * 4e-2 of the maximum (E2 .. E4).
Configs: IndexGPTConfig.small() and the two shapes of tests/test_gpu_gpt_slots.py — hidden 256 / inner 1024 (every K splits for the
matrix cores) and hidden 320 / inner 2560 (K = 320 does not split and goes group by group, K = 2560 takes the 8-way split).

E2, measured on an MI355X (worst |logit - oracle| over 12 greedy tokens; printed with -s):

    config               q8 engine    f16 engine on the dequantised blob
    small                8.785e-04    1.216e-03
    hidden 256           8.568e-04    1.234e-03
    hidden 320           1.471e-03    1.567e-03
"""
import numpy as np
import pytest

import gpt_q8_ref as Q
from mi355tts import _lib
from mi355tts import weights as W
from mi355tts.config import IndexGPTConfig
from mi355tts.indextts import IndexGPT, Sampling
from oracle import gpt_np as O

pytestmark = pytest.mark.gpu
TOL = 4e-2


def _medium(hidden, heads, inner, max_batch):
    return IndexGPTConfig(hidden=hidden, layers=2, heads=heads, inner=inner, mel_codes=301, text_tokens=64, max_mel_pos=80,
                          max_text_pos=80, max_seq=96, max_batch=max_batch, start_mel_token=299, stop_mel_token=300)


def _small(max_batch, **kw):
    return IndexGPTConfig(**{**IndexGPTConfig.small().__dict__, "max_batch": max_batch, **kw})


CONFIGS = {"small": lambda mb: _small(mb), "h256": lambda mb: _medium(256, 4, 1024, mb), "h320": lambda mb: _medium(320, 5, 2560, mb)}


def _prompt(e, cfg, seed, n_text, n_cond=4):
    conds = W.synth_normal(seed, "conds", (1, n_cond, cfg.hidden), std=0.5)
    text = (np.arange(n_text, dtype=np.int32) * 5 + seed) % (cfg.text_tokens - 2) + 2
    mh, _ = e.mel_embed(cfg.start_mel_token, 0)
    p, _ = e.concat(conds, e.text_embed(text), mh)
    return p


def _ones(cfg):
    return np.ones((1, cfg.mel_codes), np.float32)


def _teacher_forced(cfg, st, prompt, toks):
    """oracle last_hidden_state rows and logits when it is fed the engine's tokens, the penalty vector all ones"""
    keys = [np.zeros((cfg.heads, 64, 0), np.float32)] * cfg.layers
    vals = [np.zeros((cfg.heads, 0, 64), np.float32)] * cfg.layers
    pen = _ones(cfg)
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


def _oracle(name, cfg, dst, prompt, toks):
    key = (name, prompt.tobytes(), tuple(int(t) for t in toks))
    if key not in _ORACLE:
        _ORACLE[key] = _teacher_forced(cfg, dst, prompt, toks)
    return _ORACLE[key]


def _meets_bar(name, cfg, dst, prompt, toks, hid, greedy=True, what=""):
    assert len(toks) >= 1 and hid.shape == (len(toks), cfg.hidden) and np.isfinite(hid).all(), what
    ohid, ologits = _oracle(name, cfg, dst, prompt, toks)
    np.testing.assert_allclose(hid, ohid, rtol=0, atol=TOL, err_msg=str(what))
    if greedy:
        for k, t in enumerate(toks):
            assert ologits[k, t] >= ologits[k].max() - 6 * TOL, (what, k)


@pytest.fixture(scope="module", params=sorted(CONFIGS))
def world(request):
    """per config: a 64-slot q8 handle, the state, the dequantised state and blob (computed once, left unchanged)"""
    name = request.param
    cfg = CONFIGS[name](64)
    st = W.synth_state(W.gpt_spec(cfg), 13)
    blob = W.pack_gpt(cfg, st)
    e = IndexGPT(cfg, st, dtype="f16", weights="q8")
    yield name, cfg, st, Q.dequantized_state(cfg, st), W.gpt_q8_dequantized_blob(cfg, blob), e
    e.close()


def _stepwise(e, cfg, prompt, n, toks=None):
    """n tokens one call of graph E at a time (greedy, or teacher-forced with `toks`) -> tokens, last rows, logits"""
    e.reset()
    out_t, out_h, out_l = [], [], []
    hs, gl, mask = prompt, np.array([1]), 1
    for i in range(n):
        _, last, tok, logits = e.step(hs, _ones(cfg), mask, return_logits=True)
        t = int(tok[0, 0]) if toks is None else int(toks[i])
        out_t.append(t); out_h.append(last[0].copy()); out_l.append(logits[0].copy())
        hs, gl = e.mel_embed(t, gl)
        mask = 0
    return np.array(out_t), np.stack(out_h), np.stack(out_l)


def test_e1_prompt_pass_equals_the_f16_engine_on_the_dequantized_blob(world):
    name, cfg, st, dst, dblob, e = world
    f = IndexGPT(CONFIGS[name](1), blob=dblob, dtype="f16")
    try:
        for rows_text in (1, 9):                             # 4 + (n_text + 2) + 1 rows: 8 and 16
            p = _prompt(e, cfg, 5, rows_text)
            assert p.shape[1] >= 2
            e.reset(); f.reset()
            _, last_q, _ = e.step(p, _ones(cfg), 1)
            _, last_f, _ = f.step(p, _ones(cfg), 1)
            assert np.isfinite(last_q).all() and np.abs(last_q).max() > 0
            np.testing.assert_array_equal(last_q, last_f)
            for li in range(cfg.layers):
                kq, vq = e.kv_read(li)
                kf, vf = f.kv_read(li)
                assert kq.shape[2] == p.shape[1]
                np.testing.assert_array_equal(kq, kf)
                np.testing.assert_array_equal(vq, vf)
    finally:
        f.close()


def test_e2_greedy_decode_against_the_oracle_and_the_f16_engine(world):
    """module docstring: the q8 engine's weights carry no rounding the f16 engine's do not, so its worst logit error may be at
    most twice the f16 engine's (the factor covers summation order)"""
    name, cfg, st, dst, dblob, e = world
    p = _prompt(e, cfg, 7, 6)
    toks, hid, logits = _stepwise(e, cfg, p, 12)
    _meets_bar(name, cfg, dst, p, toks, hid, what=(name, "q8"))
    _, ologits = _oracle(name, cfg, dst, p, toks)
    f = IndexGPT(CONFIGS[name](1), blob=dblob, dtype="f16")
    try:
        _, fhid, flogits = _stepwise(f, cfg, p, 12, toks)
    finally:
        f.close()
    np.testing.assert_allclose(fhid, _oracle(name, cfg, dst, p, toks)[0], rtol=0, atol=TOL)
    eq, ef = float(np.abs(logits - ologits).max()), float(np.abs(flogits - ologits).max())
    print(f"\nE2 {name}: worst |logit - oracle| q8 {eq:.3e}, f16 on the dequantised blob {ef:.3e}")
    assert eq <= 2 * ef, (name, eq, ef)


@pytest.mark.parametrize("nb", [3, 12, 19, 40])
def test_e3_generate_batch(world, nb):
    name, cfg, st, dst, dblob, e = world
    saved = _lib.get_option("gpt_mfma_min")
    _lib.set_option("gpt_mfma_min", 3)                     # every index-order group of 16 has >= 3 members: the 16-column kernel
    try:
        prompts = [_prompt(e, cfg, 20 + b, 1 + (b * 5) % 7, n_cond=3) for b in range(nb)]
        limits = [5 + (b * 3) % 6 for b in range(nb)]
        res, _ = e.generate_batch(prompts, limits, stop_tokens=[], repeat_value=1.0)
        for b in range(nb):
            assert len(res[b][0]) == limits[b]
            _meets_bar(name, cfg, dst, prompts[b], res[b][0], res[b][1], what=(name, nb, b))
        if nb > 16:
            for g in range(0, nb, 16):
                gres, _ = e.generate_batch(prompts[g:g + 16], limits[g:g + 16], stop_tokens=[], repeat_value=1.0)
                for j, (t, h) in enumerate(gres):
                    np.testing.assert_array_equal(res[g + j][0], t)
                    np.testing.assert_array_equal(res[g + j][1], h)
    finally:
        _lib.set_option("gpt_mfma_min", saved)


def test_e4_the_other_entry_families(world):
    """queue (9 sentences, 4 slots), queue with 3 beams, generate_beam, the beam pool, sampled batch: each finishes, counts are
    right, and the returned hidden rows meet the bar against the oracle fed the returned tokens.  (stream_synthesize: the next test.)"""
    name, cfg, st, dst, dblob, _ = world
    cfg4 = CONFIGS[name](4)
    cfg12 = CONFIGS[name](12)
    e4 = IndexGPT(cfg4, st, dtype="f16", weights="q8")
    e12 = IndexGPT(cfg12, st, dtype="f16", weights="q8")
    try:
        prompts = [_prompt(e4, cfg4, 40 + b, 1 + b % 5, n_cond=3) for b in range(9)]
        limits = [4 + (b * 5) % 7 for b in range(9)]
        res, stats = e4.generate_queue(prompts, limits, stop_tokens=[], repeat_value=1.0, return_stats=True)
        assert len(res) == 9 and stats["steps"] >= max(limits) - 1 and stats["passes"] >= 3
        for b in range(9):
            assert len(res[b][0]) == limits[b]
            _meets_bar(name, cfg, dst, prompts[b], res[b][0], res[b][1], what=(name, "queue", b))
        res = e12.generate_queue(prompts, limits, stop_tokens=[], beams=3)
        assert len(res) == 9
        for b in range(9):
            assert len(res[b][0]) == limits[b] and np.isfinite(res[b][2])
            _meets_bar(name, cfg, dst, prompts[b], res[b][0], res[b][1], greedy=False, what=(name, "queue beams", b))
        res, _ = e12.generate_beam(prompts[:4], limits[:4], 3, stop_tokens=[])
        for b in range(4):
            assert len(res[b][0]) == limits[b] and np.isfinite(res[b][2])
            _meets_bar(name, cfg, dst, prompts[b], res[b][0], res[b][1], greedy=False, what=(name, "beam", b))
        res, _ = e12.generate_beam(prompts[:4], limits[:4], 3, stop_tokens=[], pool=True)
        for b in range(4):
            assert 1 <= len(res[b][0]) <= limits[b] and np.isfinite(res[b][2])
            _meets_bar(name, cfg, dst, prompts[b], res[b][0], res[b][1], greedy=False, what=(name, "beam pool", b))
        sp = [Sampling(1.0, 30, 0.8, 100 + b) for b in range(9)]
        res, _ = e12.generate_batch(prompts, limits, stop_tokens=[], sampling=sp)
        again, _ = e12.generate_batch(prompts, limits, stop_tokens=[], sampling=sp)          # through the captured graph
        for b in range(9):
            assert len(res[b][0]) == limits[b] and res[b][0].tolist() == again[b][0].tolist()
            _meets_bar(name, cfg, dst, prompts[b], res[b][0], res[b][1], greedy=False, what=(name, "sampled", b))
    finally:
        e4.close(); e12.close()


def test_e4_stream_synthesize(world):
    """audio while a q8 handle's queue decodes, through a small synthetic graph-F vocoder (fp32): the chunks of every sentence tile
    its waveform, and no sample is more than one LSB from the blocking pair generate_queue + run_latent_voices on the same handle
    (the bar of tests/test_gpu_indextts_stream.py); the rows that pair vocodes meet the oracle's bar"""
    import test_bigvgan_windows_layout as WL
    from mi355tts import bigvgan as BV
    from mi355tts.indextts import stream_synthesize
    name, cfg, st, dst, dblob, _ = world
    cfg4 = CONFIGS[name](4)
    limits, voice_of = [12, 5, 3, 9, 2], [0, 1, 0, 1, 0]
    vcfg = WL.small_f(num_mels=cfg.hidden)
    voices = [WL.voice(vcfg, 100), WL.voice(vcfg, 200)]
    e = IndexGPT(cfg4, st, dtype="f16", weights="q8")
    voc = BV.BigVGANVocoder(vcfg, W.synth_state(W.bigvgan_spec(vcfg), 9527), dtype="f32")
    try:
        prompts = [_prompt(e, cfg4, 60 + b, 1 + b % 4, n_cond=3) for b in range(len(limits))]
        wav, closed = {}, set()
        for i, s0, chunk, last in stream_synthesize(e, voc, prompts, limits, voices, voice_of, chunk=4, stop_tokens=[], repeat_value=1.0):
            assert i not in closed and chunk.dtype == np.int16 and chunk.size > 0 and s0 == sum(c.size for c in wav.get(i, []))
            wav.setdefault(i, []).append(chunk)
            if last:
                closed.add(i)
        assert sorted(wav) == [0, 1, 2, 3] and closed == set(wav)          # the 2-code sentence yields nothing
        rows = e.generate_queue(prompts, limits, stop_tokens=[], repeat_value=1.0)
        blocking = voc.run_latent_voices([rows[i][1] for i in sorted(wav)], voices, [voice_of[i] for i in sorted(wav)])
        for k, i in enumerate(sorted(wav)):
            w = np.concatenate(wav[i])
            assert w.size == (limits[i] - 2) * vcfg.hop + 30
            assert int(np.abs(w.astype(np.int32) - np.asarray(blocking[k]).reshape(-1).astype(np.int32)).max()) <= 1, i
            _meets_bar(name, cfg, dst, prompts[i], rows[i][0], rows[i][1], what=(name, "stream", i))
    finally:
        voc.close(); e.close()


def test_e5_error_paths():
    cfg = _small(2)
    st = W.synth_state(W.gpt_spec(cfg), 13)
    good = IndexGPT(cfg, st, dtype="f16", weights="q8")
    try:
        p = _prompt(good, cfg, 3, 4)
        before, _ = good.generate_batch([p], [5], stop_tokens=[])
        with pytest.raises(_lib.MiError, match="MI_F32"):
            IndexGPT(cfg, st, dtype="f32", weights="q8")
        with pytest.raises(_lib.MiError, match="MI_BF16"):
            IndexGPT(cfg, st, dtype="bf16", weights="q8")
        bad = IndexGPTConfig(**{**cfg.__dict__, "inner": 136})
        with pytest.raises(_lib.MiError, match="multiples of 16"):
            IndexGPT(bad, W.synth_state(W.gpt_spec(bad), 13), dtype="f16", weights="q8")
        odd = IndexGPTConfig(**{**cfg.__dict__, "hidden": 136})          # not heads * 64 either: refused whatever the format
        with pytest.raises(_lib.MiError):
            IndexGPT(odd, W.synth_state(W.gpt_spec(odd), 13), dtype="f16", weights="q8")
        with pytest.raises(ValueError):
            IndexGPT(cfg, st, dtype="f16", weights="q4")
        L = _lib.load()
        q, s, z = np.zeros((8, 24), np.uint8), np.ones(8, np.float32), np.zeros(8, np.uint8)
        x, out = np.zeros((2, 24), np.float32), np.zeros((2, 8), np.float32)
        rc = L.mi_gpt_linear_decode_q8(q.ctypes.data, s.ctypes.data, z.ctypes.data, None, x.ctypes.data, _lib.DTYPES["f16"], 8, 24,
                                       None, None, None, None, None, None, 0, 1, 0, 0, 1, None, None, out.ctypes.data, _lib.MI_HOST)
        assert rc == _lib.MI_EINVAL and b"multiple of 16" in L.mi_last_error()
        rc = L.mi_gpt_linear_batch_q8(q.ctypes.data, s.ctypes.data, z.ctypes.data, None, x.ctypes.data, None, _lib.DTYPES["f16"], 8, 24,
                                      2, None, 0, 1, 0, None, 1, None, None, out.ctypes.data, _lib.MI_HOST)
        assert rc == _lib.MI_EINVAL and b"multiple of 16" in L.mi_last_error()
        assert L.mi_gpt_weight_bytes(None) < 0
        after, _ = good.generate_batch([p], [5], stop_tokens=[])
        assert after[0][0].tolist() == before[0][0].tolist()
        np.testing.assert_array_equal(after[0][1], before[0][1])
        other = IndexGPT(cfg, st, dtype="f32")
        t, _, _ = other.generate_from_prompt(p, 5, stop_tokens=[], repeat_penality=_ones(cfg))
        assert len(t) == 5
        other.close()
    finally:
        good.close()


def test_e7_the_three_construction_routes_hold_the_same_bytes():
    """state, host blob and device blob: quantised on the host from the same fp32 values whichever route — the same prompt pass and
    the same first decode steps, bit for bit"""
    import torch
    cfg = _small(2)
    st = W.synth_state(W.gpt_spec(cfg), 13)
    blob = W.pack_gpt(cfg, st)
    outs = []
    for kw in (dict(state=st), dict(blob=blob), dict(blob_device=torch.from_numpy(blob).cuda())):
        e = IndexGPT(cfg, dtype="f16", weights="q8", **kw)
        try:
            p = _prompt(e, cfg, 5, 4)
            toks, hid, logits = _stepwise(e, cfg, p, 4)
            outs.append((toks, hid, logits, e.kv_read(0), e.weight_bytes()))
        finally:
            e.close()
    for o in outs[1:]:
        np.testing.assert_array_equal(o[0], outs[0][0])
        np.testing.assert_array_equal(o[1], outs[0][1])
        np.testing.assert_array_equal(o[2], outs[0][2])
        np.testing.assert_array_equal(o[3][0], outs[0][3][0])
        np.testing.assert_array_equal(o[3][1], outs[0][3][1])
        assert o[4] == outs[0][4]


def test_e6_weight_bytes(world):
    name, cfg, st, dst, dblob, e = world
    h, n, c = cfg.hidden, cfg.inner, cfg.mel_codes
    mats = [(3 * h, h), (h, h), (n, h), (h, n)] * cfg.layers + [(c, h)]
    elems, rows = sum(a * b for a, b in mats), sum(a for a, _ in mats)
    scratch = 2 * max(a * b for a, b in mats)
    assert e.weight_bytes() == elems + 4 * rows + rows + scratch
    f = IndexGPT(CONFIGS[name](1), st, dtype="f16")
    try:
        assert f.weight_bytes() == 2 * elems
    finally:
        f.close()
