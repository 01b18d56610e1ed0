"""GPU: ragged F5 batches — utterances of different prompt, text and max_duration in one sampling loop (padded slabs of
Nmax = max N_u rows, a device length table; include/mi355tts.h mi_f5_synthesize_ragged / mi_f5_dit_eval_ragged).

  * equal lengths through the ragged entry == the uniform entry, bit for bit, with the length-aware kernels engaged;
  * every utterance of a ragged DiT evaluation against the float64 oracle at its own N, in every arithmetic form, and with
    forced key slices (whole slices past an utterance's length publish the neutral partial);
  * isolation: changing one utterance leaves the others' pred bit-identical (attention and the position convolution are
    the only places rows meet);
  * full size end to end: the north-star utterance within the reference gate, every utterance == itself alone;
  * one captured graph serves every length mix of a (U, Nmax); argument errors leave the handle usable.
"""
import dataclasses
import os

import numpy as np
import pytest

from mi355tts import _lib
from mi355tts import weights as W
from mi355tts.config import F5Config
from mi355tts.f5 import F5Engine
from oracle import f5_np as O

from dit_oracle64 import F32_OVERALL_GATE, F32_ROW_GATE, dit_errors, dit_forward64, rms, widen

pytestmark = pytest.mark.gpu

K_EVAL = 2
ATTN_SPLIT_DEFAULT = 2          # "attn_split" of the fp32 128-query kernel (the library default; pinned in tests/test_options.py)
LONG = (701, 1037, 1153)        # the exact-fit tiling's boundaries (test_gpu_dit_tilings) as one batch
SHORT = (67, 130, 257)          # one to five 64-key stages: forced key slices run wholly past the short utterances


def _mid_cfg(**kw):
    """test_gpu_dit_tilings._mid_cfg: full-width DiT layers, two blocks, small front / back end."""
    return F5Config(depth=2, text_dim=64, text_num_embeds=40, conv_layers=1, vocos_dim=64, vocos_intermediate=128, vocos_layers=1,
                    nfe_step=4, **kw)


def _utt(cfg, N, u, seed=3):
    """test_gpu_dit_tilings._inputs, utterance u at N frames."""
    cd = cfg.mel_dim + cfg.text_dim
    return (W.synth_normal(seed + u, f"n{N}", (N, cfg.mel_dim)), W.synth_normal(seed + 11 + u, f"c{N}", (N, cd), std=0.7),
            W.synth_normal(seed + 22 + u, f"d{N}", (N, cd), std=0.7))


@pytest.fixture(scope="module")
def mid():
    cfg = _mid_cfg()
    raw = W.synth_state(W.f5_spec(cfg), 7)
    st = W.fold_f5(cfg, raw)
    return cfg, raw, widen(st), O.time_tables(cfg, st)[2][K_EVAL], {}


def _batch(mid, lengths):
    """inputs of utterance u at lengths[u], and their float64 references (cached per (N, u) for the module)."""
    cfg, _, st64, t_emb, cache = mid
    ins = [_utt(cfg, N, u) for u, N in enumerate(lengths)]
    refs = []
    for u, N in enumerate(lengths):
        if (N, u) not in cache:
            with pytest.MonkeyPatch.context() as mp:
                cache[(N, u)] = dit_forward64(mp, cfg, st64, *ins[u], t_emb)
        refs.append(cache[(N, u)])
    return [i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins], refs


def _ragged_profiled(eng, x, c, d):
    _lib.prof_reset(); _lib.prof_enable(("attn",))
    try:
        p = eng.dit_eval_ragged(x, c, d, K_EVAL)
    finally:
        _lib.prof_enable(())
    return p, {k["kernel"] for k in _lib.prof_kernels() if k["launches"] > 0}


F32_FORMS = {
    "pairs-fold": dict(f32_arithmetic="fp16x2-pairs"),
    "pairs-rownorm": dict(f32_arithmetic="fp16x2-pairs", adaln_fold=False),
    "bf16x3": dict(f32_arithmetic="bf16x3"),
    "native": dict(f32_arithmetic="native-fp32-mfma"),
}


# ---------------------------------------------------------------------------------------------
# equal lengths: the ragged entry (length-aware kernels) against the uniform entry, bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_equal_lengths_match_the_uniform_batch_bit_for_bit(mid, dtype):
    cfg, raw = mid[0], mid[1]
    eng = F5Engine(cfg, raw, dtype=dtype)
    try:
        for N in (1037, 257):
            x, c, d = (np.stack(a) for a in zip(*[_utt(cfg, N, u) for u in range(3)]))
            uni = eng.dit_eval(x, c, d, K_EVAL)
            rag, kernels = _ragged_profiled(eng, list(x), list(c), list(d))
            assert any(k.endswith(" + lengths") for k in kernels), kernels      # the VARLEN attention ran
            for u in range(3):
                assert rag[u].shape == (2, N, cfg.mel_dim)
                assert np.array_equal(rag[u], uni[2 * u:2 * u + 2]), (dtype, N, u)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------
# every utterance of a ragged evaluation against the float64 oracle at its own length
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(F32_FORMS))
@pytest.mark.parametrize("lengths", [LONG, SHORT])
def test_fp32_ragged_against_float64_oracle(mid, form, lengths):
    cfg, raw = mid[0], mid[1]
    x, c, d, refs = _batch(mid, lengths)
    eng = F5Engine(dataclasses.replace(cfg, **F32_FORMS[form]), raw, dtype="f32")
    try:
        pred = eng.dit_eval_ragged(x, c, d, K_EVAL)
        assert eng.info()["saturation_events"] == 0
    finally:
        eng.close()
    for u, N in enumerate(lengths):
        assert pred[u].shape == (2, N, cfg.mel_dim) and np.isfinite(pred[u]).all()
        ea, er = dit_errors(pred[u], refs[u])
        print(f"{form} {lengths} u={u}: rel rms {ea:.2e}, worst row {er:.2e}")
        assert ea < F32_OVERALL_GATE and er < F32_ROW_GATE, (form, lengths, u, ea, er)


# gates of test_gpu_f5.test_dit_16bit_ragged_batch_against_oracle (rel rms, and max |err| < 12 x that x rms(ref))
@pytest.mark.parametrize("dtype,ref_fp16,tol", [("f16", False, 1.5e-2), ("bf16", False, 8e-2), ("f16", True, 1.5e-2)])
@pytest.mark.parametrize("lengths", [LONG, SHORT])
def test_16bit_ragged_against_float64_oracle(mid, dtype, ref_fp16, tol, lengths):
    cfg, raw = mid[0], mid[1]
    x, c, d, refs = _batch(mid, lengths)
    eng = F5Engine(dataclasses.replace(cfg, ref_fp16_attn=ref_fp16), raw, dtype=dtype)
    try:
        pred = eng.dit_eval_ragged(x, c, d, K_EVAL)
    finally:
        eng.close()
    for u, N in enumerate(lengths):
        assert pred[u].shape == (2, N, cfg.mel_dim) and np.isfinite(pred[u]).all()
        e = rms(pred[u] - refs[u]) / rms(refs[u])
        print(f"{dtype} ref_fp16={ref_fp16} {lengths} u={u}: rel rms {e:.2e}")
        assert e < tol and np.abs(pred[u] - refs[u]).max() < 12 * tol * rms(refs[u]), (dtype, ref_fp16, lengths, u, e)


@pytest.mark.parametrize("split,z,lengths", [(ATTN_SPLIT_DEFAULT, 2, SHORT), (ATTN_SPLIT_DEFAULT, 3, SHORT), (ATTN_SPLIT_DEFAULT, 4, SHORT),
                                             (1, 4, SHORT), (0, 0, LONG), (1, 0, LONG)])
def test_key_slices_past_an_utterance_publish_the_neutral_partial(mid, split, z, lengths):
    """attn_z_force = z: exactly z key slices even where an utterance has fewer 64-key stages (N = 67: two stages, so two of
    four slices hold no key of it); the merge must turn them into the unsliced result, and every ticket counter must be back
    at zero for the next launch (the second evaluation below reuses them)."""
    cfg, raw = mid[0], mid[1]
    x, c, d, refs = _batch(mid, lengths)
    eng = F5Engine(cfg, raw, dtype="f32")
    saved = {k: _lib.get_option(k) for k in ("attn_z_force", "attn_split")}
    try:
        _lib.set_option("attn_split", split)
        _lib.set_option("attn_z_force", z)
        a = eng.dit_eval_ragged(x, c, d, K_EVAL)
        b = eng.dit_eval_ragged(x, c, d, K_EVAL)
    finally:
        for k, v in saved.items():
            _lib.set_option(k, v)
        eng.close()
    for u in range(len(lengths)):
        assert np.array_equal(a[u], b[u]), u
        ea, er = dit_errors(a[u], refs[u])
        assert ea < F32_OVERALL_GATE and er < F32_ROW_GATE, (split, z, lengths, u, ea, er)


# ---------------------------------------------------------------------------------------------
# isolation: nothing of utterance 1 reaches utterances 0 and 2
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("lengths", [LONG, (257, 67, 130)])
def test_other_utterances_do_not_leak_in(mid, dtype, lengths):
    cfg, raw = mid[0], mid[1]
    x, c, d = (list(a) for a in zip(*[_utt(cfg, N, u) for u, N in enumerate(lengths)]))
    eng = F5Engine(cfg, raw, dtype=dtype)
    try:
        a = eng.dit_eval_ragged(x, c, d, K_EVAL)
        n1 = lengths[1]
        x[1], c[1], d[1] = (3.0 * v for v in _utt(cfg, n1, 7))
        b = eng.dit_eval_ragged(x, c, d, K_EVAL)
    finally:
        eng.close()
    assert not np.array_equal(a[1], b[1])
    for u in (0, 2):
        assert np.array_equal(a[u], b[u]), (dtype, lengths, u)


# ---------------------------------------------------------------------------------------------
# one graph per (U, Nmax) for every length mix; errors leave the handle usable (mid config: 3 sampling steps)
# ---------------------------------------------------------------------------------------------
def _mid_request(cfg, u, L, T):
    t = np.arange(L) / cfg.sample_rate
    a = 0.1 * 32767 * np.sin(2 * np.pi * (180 + 40 * u) * t) + W.synth_normal(50 + u, "audio", (L,), std=500.0)
    ids = (np.arange(T) * (7 + u)) % (cfg.text_num_embeds - 1)
    return np.clip(np.round(a), -32768, 32767).astype(np.int16), ids.astype(np.int32)


def _close_lsb(a, b):
    d = np.abs(a.astype(np.int32) - b.astype(np.int32))
    return a.shape == b.shape and d.max(initial=0) <= 2 and (d > 0).mean() < 0.01


def test_one_graph_serves_every_length_mix(mid):
    cfg, raw = mid[0], mid[1]
    eng = F5Engine(cfg, raw, dtype="f32")
    reqs = [_mid_request(cfg, u, L, T) for u, (L, T) in enumerate([(25600, 40), (38400, 60)])]
    audios, ids = [r[0] for r in reqs], [r[1] for r in reqs]
    try:
        outs = []
        for Ns in ([400, 300], [250, 400], [400, 333]):            # eager, capture, replay: one (U, Nmax)
            w = eng.synthesize_ragged(audios, ids, Ns)
            for u in range(2):
                alone = eng.synthesize(audios[u][None], ids[u][None], Ns[u], seed=9527 + u)
                assert w[u].shape == (1, (Ns[u] - cfg.ref_frames(audios[u].size) - 1) * cfg.hop_length) == alone[0].shape
                assert _close_lsb(w[u], alone[0]), (Ns, u)
                assert rms(w[u].astype(np.float64)) > 0
            outs.append(w)
        again = eng.synthesize_ragged(audios, ids, [400, 333])
        for u in range(2):
            assert np.array_equal(again[u], outs[2][u]), u
        assert eng.info()["saturation_events"] == 0
    finally:
        eng.close()


def _raw(eng, audios, ids, Ns, out_cap=None, U=None):
    a = np.ascontiguousarray(np.concatenate(audios))
    t = np.ascontiguousarray(np.concatenate(ids).astype(np.int32))
    al = np.asarray([x.size for x in audios], np.int64)
    tl = np.asarray([x.size for x in ids], np.int64)
    nl = np.asarray(Ns, np.int64)
    cap = 1 << 22 if out_cap is None else out_cap
    out = np.zeros(max(cap, 1), np.int16)
    ol = np.zeros(len(audios), np.int64)
    return _lib.load().mi_f5_synthesize_ragged(eng._h, len(audios) if U is None else U, a.ctypes.data, al.ctypes.data, t.ctypes.data,
                                               tl.ctypes.data, nl.ctypes.data, None, 9527, out.ctypes.data, cap, ol.ctypes.data,
                                               _lib.MI_HOST)


def test_argument_errors_leave_the_handle_usable(mid):
    cfg, raw = mid[0], mid[1]
    eng = F5Engine(cfg, raw, dtype="f32")
    reqs = [_mid_request(cfg, u, L, T) for u, (L, T) in enumerate([(25600, 40), (38400, 60), (12800, 20)])]
    audios, ids = [r[0] for r in reqs], [r[1] for r in reqs]
    Ns = [300, 400, 200]
    R = [cfg.ref_frames(a.size) for a in audios]
    try:
        good = eng.synthesize_ragged(audios, ids, Ns)
        total = sum((n - r - 1) * cfg.hop_length for n, r in zip(Ns, R))
        bad_ids = [ids[0], ids[1], ids[2].copy()]
        bad_ids[2][5] = 10 ** 6
        cases = {
            "no generated frame": dict(Ns=[300, R[1], 200]),
            "text longer than N": dict(Ns=[300, 400, 15]),
            "N above max_signal_length": dict(Ns=[300, cfg.max_signal_length + 1, 200]),
            "out_cap too small": dict(out_cap=total - 1),
            "U < 1": dict(U=0),
        }
        for name, kw in cases.items():
            rc = _raw(eng, audios, ids, kw.get("Ns", Ns), out_cap=kw.get("out_cap"), U=kw.get("U"))
            assert rc == -1, (name, rc)                                      # MI_EINVAL
            w = eng.synthesize_ragged(audios, ids, Ns)
            assert all(_close_lsb(a, b) for a, b in zip(w, good)), name
        assert _raw(eng, audios, bad_ids, Ns) == -1                    # text id out of range in utterance 2
        with pytest.raises(_lib.MiError):
            eng.synthesize_ragged(audios, bad_ids, Ns)
        w = eng.synthesize_ragged(audios, ids, Ns)
        assert all(_close_lsb(a, b) for a, b in zip(w, good))
        assert eng.info()["saturation_events"] == 0
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------
# full size (F5Config(), BASELINE weights), U = 3 of three different shapes
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full3():
    cfg = F5Config()
    raw = W.synth_state(W.f5_spec(cfg), 9527)
    a0, i0, N0, n0 = W.f5_synthetic_inputs(cfg, 8, 0)                          # utterance 0 = the north-star input
    a1, i1, N1, n1 = W.f5_synthetic_inputs(cfg, 1, first=1, L=162240)          # the reference prompt's 6.76 s
    a2, i2, _, _ = W.f5_synthetic_inputs(cfg, 1, first=2, L=89600)             # a short prompt and a short text
    N2 = 700
    n2 = W.synth_normal(9529, "noise", (N2, cfg.mel_dim))
    audios, ids, Ns, noise = [a0[0], a1[0], a2[0]], [i0[0], i1[0], i2[0, :60]], [N0, N1, N2], [n0[0], n1[0], n2]
    return cfg, raw, audios, ids, Ns, noise


def test_full_size_ragged_batch_end_to_end(full3, golden_dir):
    cfg, raw, audios, ids, Ns, noise = full3
    assert Ns[0] == 1126 and Ns[1] == 1268 and audios[1].size == 162240
    gfull = np.load(os.path.join(golden_dir, "f5_full.npz"))
    e32 = F5Engine(cfg, raw, dtype="f32")
    try:
        w = e32.synthesize_ragged(audios, ids, Ns, noise=noise)
        for u in range(3):
            R = cfg.ref_frames(audios[u].size)
            assert w[u].dtype == np.int16 and w[u].shape == (1, (Ns[u] - R - 1) * cfg.hop_length)
        err = rms((w[0][0].astype(np.float64) - gfull["e2e_i16"].astype(np.float64)) / 32767.0)
        assert w[0].shape[1] == gfull["e2e_i16"].shape[0] and err < 1e-3, err             # the north-star gate
        for u in range(3):
            alone = e32.synthesize(audios[u][None], ids[u][None], Ns[u], noise=noise[u][None])
            assert _close_lsb(w[u], alone[0]), u
            assert rms(w[u].astype(np.float64)) > 300
        assert e32.info()["saturation_events"] == 0
    finally:
        e32.close()
    e16 = F5Engine(cfg, raw, dtype="bf16")
    try:
        wb = e16.synthesize_ragged(audios, ids, Ns, noise=noise)
    finally:
        e16.close()
    for u in range(3):
        e = rms((wb[u].astype(np.float64) - w[u].astype(np.float64)) / 32767.0)
        print(f"full size ragged u={u} N={Ns[u]}: bf16 vs fp32 waveform rms {e:.2e}")
        assert e < 1.5e-3, (u, e)
