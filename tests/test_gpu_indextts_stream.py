"""GPU: audio while the queue decodes (indextts.stream_synthesize): a queue session on the GPT, and after every round ONE windowed
graph-F forward over everything indextts.stream_plan reports ready, reading the rows from the session's device tensor.

Seven sentences with limits (100, 61, 3, 2, 1, 90, 47) through three slots, no stop ids, two voices alternating, chunk 8, the
structural halo (39).  The reference is the numpy oracle fed the rows the blocking queue produces, which are the session's bit for
bit (tests/test_gpu_gpt_queue_session.py).  Gates: fp32 vocoder 1e-5 rms (the stream yields int16, so its gate is on int16 / 32767
against the oracle's int16, and no sample may be more than one LSB from the blocking pair's), f16 vocoder 2e-2."""
import numpy as np
import pytest

import test_bigvgan_windows_layout as WL
from mi355tts import weights as W
from mi355tts import bigvgan as BV
from mi355tts.config import IndexGPTConfig
from mi355tts.indextts import IndexGPT, stream_synthesize
from oracle import bigvgan_np as O

pytestmark = pytest.mark.gpu
LIMITS = (100, 61, 3, 2, 1, 90, 47)
VOICE_OF = (0, 1, 0, 1, 0, 1, 0)
CHUNK = 8


class Spy:
    """an IndexGPT whose sessions log the counts every advance() reports"""

    def __init__(self, gpt):
        self._gpt, self.cfg, self.log = gpt, gpt.cfg, []

    def queue_session(self, *a, **kw):
        q = self._gpt.queue_session(*a, **kw)
        adv, log = q.advance, self.log

        def advance():
            r = adv()
            log.append(r[0].copy())
            return r
        q.advance = advance
        return q


@pytest.fixture(scope="module")
def env():
    cfg = IndexGPTConfig(hidden=256, layers=2, heads=4, inner=1024, mel_codes=301, text_tokens=64, max_mel_pos=120, max_text_pos=80,
                         max_seq=160, max_batch=3, start_mel_token=299, stop_mel_token=300)
    gpt = IndexGPT(cfg, W.synth_state(W.gpt_spec(cfg), 17), dtype="f32")
    vcfg = WL.small_f(num_mels=256)
    vst = W.synth_state(W.bigvgan_spec(vcfg), 9527)
    voices = [WL.voice(vcfg, 100), WL.voice(vcfg, 200)]
    mh, _ = gpt.mel_embed(cfg.start_mel_token, 0)
    prompts = []
    for b in range(len(LIMITS)):
        conds = W.synth_normal(40 + b, "conds", (1, 4, cfg.hidden), std=0.5)
        text = (np.arange(3 + b, dtype=np.int32) * 5 + b) % (cfg.text_tokens - 2) + 2
        prompts.append(gpt.concat(conds, gpt.text_embed(text), mh)[0])
    rows = gpt.generate_queue(prompts, list(LIMITS), stop_tokens=[])
    assert [len(t) for t, _ in rows] == list(LIMITS)
    # the oracle on the final rows, once, shared and never written to
    ref = {i: O.indextts_f_float(vcfg, vst, h, voices[VOICE_OF[i]]).reshape(-1) for i, (_, h) in enumerate(rows) if LIMITS[i] >= 3}
    for r in ref.values():
        r.setflags(write=False)

    class E:
        pass
    e = E()
    e.cfg, e.gpt, e.vcfg, e.vst, e.voices, e.prompts, e.rows, e.ref = cfg, gpt, vcfg, vst, voices, prompts, rows, ref
    yield e
    gpt.close()


def _stream(env, voc, spy=None):
    """the stream, assembled: per sentence the chunks must tile [0, F * hop + 30) in order, `last` on the final one only"""
    wav, closed, first_round = {}, set(), {}
    for i, s0, chunk, last in stream_synthesize(spy or env.gpt, voc, env.prompts, list(LIMITS), env.voices, VOICE_OF, chunk=CHUNK,
                                                stop_tokens=[]):
        assert i not in closed and chunk.dtype == np.int16 and chunk.size > 0
        assert s0 == sum(c.size for c in wav.get(i, []))
        wav.setdefault(i, []).append(chunk)
        if spy is not None and i not in first_round:
            first_round[i] = int(spy.log[-1][i])
        if last:
            closed.add(i)
    out = {i: np.concatenate(c) for i, c in wav.items()}
    assert closed == set(out)
    for i, w in out.items():
        assert w.size == (LIMITS[i] - 2) * env.vcfg.hop + 30
    return out, {i: len(c) for i, c in wav.items()}, first_round


def test_stream_fp32(env):
    voc = BV.BigVGANVocoder(env.vcfg, env.vst, dtype="f32")
    try:
        spy = Spy(env.gpt)
        out, n_chunks, first_round = _stream(env, voc, spy)
        assert sorted(out) == [0, 1, 2, 5, 6]                     # the 1- and 2-code sentences yield nothing
        assert out[2].size == env.vcfg.hop + 30 and n_chunks[2] == 1
        # sentence 0's first chunk arrives while it is still decoding, and it arrives in pieces
        print("counts at the first chunk:", first_round, "chunks:", n_chunks)
        assert first_round[0] < 100 and n_chunks[0] > 2
        blocking, blocking_f = voc.run_latent_voices([env.rows[i][1] for i in sorted(out)], env.voices, [VOICE_OF[i] for i in sorted(out)],
                                                     return_float=True)
        for k, i in enumerate(sorted(out)):
            ref = env.ref[i]
            e_blk = WL.rms(blocking_f[k].reshape(-1) - ref)
            ref_i16 = (np.clip(ref, -1.0, 1.0) * np.float32(32767.0)).astype(np.int16)
            e_str = WL.rms((out[i].astype(np.float64) - ref_i16) / 32767.0)
            d = int(np.abs(out[i].astype(np.int32) - blocking[k].reshape(-1).astype(np.int32)).max())
            print(f"sentence {i}: blocking pair float rms {e_blk:.3e}; stream int16 rms vs the oracle {e_str:.3e}, max |stream - blocking| {d} LSB")
            assert e_blk < 1e-5
            assert e_str < 1e-5 and d <= 1
    finally:
        voc.close()


def test_stream_f16_vocoder(env):
    """the same stream with an f16 vocoder (the GPT stays fp32, so the rows and the oracle are the shared ones)"""
    voc = BV.BigVGANVocoder(env.vcfg, env.vst, dtype="f16")
    try:
        out, _, _ = _stream(env, voc)
        assert sorted(out) == [0, 1, 2, 5, 6]
        for i in sorted(out):
            ref_i16 = (np.clip(env.ref[i], -1.0, 1.0) * np.float32(32767.0)).astype(np.int16)
            e16 = WL.rms((out[i].astype(np.float64) - ref_i16) / 32767.0)
            print(f"sentence {i}: f16 int16 rms {e16:.3e}")
            assert e16 < 2e-2
    finally:
        voc.close()
