"""GPU: audio while the queue decodes in pool mode (indextts.stream_synthesize(..., beams=B, pool=True, sampling=...)): upstream
IndexTTS' decode configuration (3 beams, sampled, top_k 30, top_p 0.8, length_penalty 0) streamed.  No row of a sentence is final
before its search ends, so the session reports a sentence's count as 0 until its group is retired and stream_plan then emits it
whole: audio leaves sentence by sentence while the other groups go on decoding.

Seven sentences with limits (30, 17, 3, 2, 1, 25, 12) through the two groups of a seven-slot engine at 3 beams (one slot never
run), no stop ids — every search then runs to its limit and returns that many codes —, two voices alternating, the small vocoder
of tests/test_gpu_indextts_stream.py.  Every chunk has to be a whole sentence, and its samples have to be those of
run_latent_voices over the rows generate_queue(beams=3, pool=True, sampling=...) gives: the same rows (the session's arrays are the
blocking entry's bit for bit) through the same forward of the whole sentence."""
import numpy as np
import pytest

import test_bigvgan_windows_layout as WL
from mi355tts import weights as W
from mi355tts import bigvgan as BV
from mi355tts.config import IndexGPTConfig
from mi355tts.indextts import IndexGPT, Sampling, stream_synthesize

pytestmark = pytest.mark.gpu
LIMITS = (30, 17, 3, 2, 1, 25, 12)
VOICE_OF = (0, 1, 0, 1, 0, 1, 0)
KW = dict(repeat_value=0.7, penalty_range=3)


@pytest.mark.parametrize("sampled", [True, False], ids=["sampled", "deterministic"])
def test_stream_in_pool_mode_emits_whole_sentences(sampled):
    cfg = IndexGPTConfig(hidden=256, layers=2, heads=4, inner=1024, mel_codes=301, text_tokens=64, max_mel_pos=120, max_text_pos=80,
                         max_seq=160, max_batch=7, start_mel_token=299, stop_mel_token=300)
    gpt = IndexGPT(cfg, W.synth_state(W.gpt_spec(cfg), 17), dtype="f32")
    vcfg = WL.small_f(num_mels=256)
    voc = BV.BigVGANVocoder(vcfg, W.synth_state(W.bigvgan_spec(vcfg), 9527), dtype="f32")
    try:
        voices = [WL.voice(vcfg, 100), WL.voice(vcfg, 200)]
        mh, _ = gpt.mel_embed(cfg.start_mel_token, 0)
        prompts = []
        for b in range(len(LIMITS)):
            conds = W.synth_normal(40 + b, "conds", (1, 4, cfg.hidden), std=0.5)
            text = (np.arange(3 + b, dtype=np.int32) * 5 + b) % (cfg.text_tokens - 2) + 2
            prompts.append(gpt.concat(conds, gpt.text_embed(text), mh)[0])
        kw = dict(stop_tokens=[], beams=3, pool=True, length_penalty=0.0,
                  sampling=[Sampling(1.0, 30, 0.8, 1001 + i) for i in range(len(LIMITS))] if sampled else None, **KW)
        rows = gpt.generate_queue(prompts, list(LIMITS), **kw)
        assert [len(t) for t, _, _ in rows] == list(LIMITS)
        order, wav = [], {}
        for i, s0, chunk, last in stream_synthesize(gpt, voc, prompts, list(LIMITS), voices, VOICE_OF, chunk=8, **kw):
            assert i not in wav and s0 == 0 and last and chunk.dtype == np.int16           # one chunk: the whole sentence
            assert chunk.size == (LIMITS[i] - 2) * vcfg.hop + 30
            wav[i] = chunk
            order.append(i)
        assert sorted(wav) == [0, 1, 2, 5, 6]                         # the 1- and 2-code sentences yield nothing
        # sentences leave as their groups retire, not at the end and not in index order: the short ones overtake sentence 0
        print("order of the chunks:", order)
        assert order.index(1) < order.index(0) and order.index(2) < order.index(0)
        blocking = voc.run_latent_voices([rows[i][1] for i in sorted(wav)], voices, [VOICE_OF[i] for i in sorted(wav)])
        for k, i in enumerate(sorted(wav)):
            d = int(np.abs(wav[i].astype(np.int32) - blocking[k].reshape(-1).astype(np.int32)).max())
            print(f"sentence {i}: max |stream - blocking| {d} LSB over {wav[i].size} samples")
            np.testing.assert_array_equal(wav[i], blocking[k].reshape(-1))
    finally:
        voc.close()
        gpt.close()
