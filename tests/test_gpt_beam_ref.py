"""CPU: the beam search reference (tests/gpt_beam_ref.py) against the definition's corner cases and the numpy oracle's greedy loop,
the borderline share of the unit inputs the GPU tests use, and the Python argument checks of the ``beams`` keyword."""
import numpy as np
import pytest

import gpt_beam_ref as R
from mi355tts import weights as W
from mi355tts.config import IndexGPTConfig
from mi355tts.indextts import IndexGPT, Sampling
from oracle import gpt_np as O

SEED = 9527


@pytest.fixture(scope="module")
def small():
    cfg = IndexGPTConfig.small()
    st = W.synth_state(W.gpt_spec(cfg), SEED)
    return cfg, st, R.OracleModel(cfg, st)


def _oracle_prompt(cfg, st, seed, n_text=6, n_cond=4):
    conds = W.synth_normal(seed, "conds", (1, n_cond, cfg.hidden), std=0.5)
    text = (np.arange(n_text, dtype=np.int32) * 5 + seed) % (cfg.text_tokens - 2) + 2
    mh, _ = O.graph_c(cfg, st, [[cfg.start_mel_token]], [0])
    p, _ = O.graph_d(conds, O.graph_b(cfg, st, text), mh)
    return conds, text, p


def test_one_beam_is_the_oracles_greedy_loop(small):
    cfg, st, model = small
    for seed in (1, 2):
        conds, text, p = _oracle_prompt(cfg, st, seed)
        toks, hid, pen = O.generate(cfg, st, conds, text, max_generate_length=p.shape[1] + 24, stop_tokens=[])
        r = R.beam_generate(model, p, 1, 24, repeat_value=cfg.repeat_penalty, penalty_range=cfg.penalty_range)
        assert r["tokens"] == toks and len(toks) == 24
        np.testing.assert_array_equal(r["hidden"], hid)
        np.testing.assert_array_equal(r["pen"], pen[0])
        # with a stop id the greedy loop ends on it, the token counted and not penalised
        stop = toks[7]
        first = toks.index(stop)
        ts, hs, ps = O.generate(cfg, st, conds, text, max_generate_length=p.shape[1] + 24, stop_tokens=[stop])
        rs = R.beam_generate(model, p, 1, 24, stop_tokens=[stop], repeat_value=cfg.repeat_penalty,
                             penalty_range=cfg.penalty_range)
        assert rs["tokens"] == ts == toks[: first + 1]
        np.testing.assert_array_equal(rs["pen"], ps[0])


def test_select_tie_rule():
    for beams in (1, 2, 3, 5, 8):
        lg, prev = R.tie_rows(beams)
        codes = lg.shape[1]
        for first in (True, False):
            par, tok, sc, margin = R.select(lg, None, prev, beams, first)
            rows = 1 if first else beams
            z = lg[:rows].astype(np.float64)
            lp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
            cand = (lp if first else lp + prev[:, None].astype(np.float64)).reshape(-1)
            want = sorted(range(cand.size), key=lambda i: (-cand[i], i))[:beams]      # descending, lower flat index first
            assert (par * codes + tok).tolist() == want
            assert margin == 0.0 or margin >= 0.2                                    # exact ties or a whole step of 0.25
            np.testing.assert_allclose(sc, cand[want], rtol=0, atol=1e-12)
            if not first and beams > 1:
                assert par[0] == 0 and len(set(par.tolist())) > 1                    # identical rows: the tie crosses rows


def test_select_penalty_and_first_row_only():
    rng = np.random.default_rng(3)
    lg = (3 * rng.standard_normal((3, 50))).astype(np.float32)
    pen = np.where(rng.random((3, 50)) < 0.3, 0.7, 1.0).astype(np.float32)
    par, tok, sc, _ = R.select(lg, pen, None, 3, True)
    z = (lg[0] * pen[0]).astype(np.float32).astype(np.float64)
    lp = z - np.log(np.exp(z).sum())
    assert par.tolist() == [0, 0, 0] and tok.tolist() == np.argsort(-lp, kind="stable")[:3].tolist()
    bad = lg.copy()
    bad[1:] = np.nan
    par2, tok2, sc2, _ = R.select(bad, pen, None, 3, True)
    assert tok2.tolist() == tok.tolist() and sc2.tolist() == sc.tolist()


class _Scripted:
    """a model whose logits are a table: step n of a hypothesis whose last token is t gives rows[n][t]"""

    def __init__(self, rows):
        self.rows = rows

    def prompt(self, prompt):
        return self.rows[0][0], np.zeros(2, np.float32), 0

    def step(self, kv, token, gen_len):
        return self.rows[gen_len][token], np.full(2, gen_len, np.float32), gen_len


def _scripted_rows(steps, codes=6):
    rng = np.random.default_rng(11)
    return [[(2 * rng.standard_normal(codes)).astype(np.float32) for _ in range(codes)] for _ in range(steps)]


def test_stop_on_another_hypothesis_keeps_going_and_on_hypothesis_0_ends():
    rows = _scripted_rows(12)
    free = R.beam_generate(_Scripted(rows), None, 2, 10, penalty_range=3)
    assert len(free["tokens"]) == 10 and len(free["top_tokens"]) == 10
    # hypothesis 1's first token as the stop id: hypothesis 0 does not carry it there, so nothing ends at selection 0
    par, tok, _, _ = R.select(rows[0][0][None], None, None, 2, True)
    stop = int(tok[1])
    assert stop != free["top_tokens"][0]
    r = R.beam_generate(_Scripted(rows), None, 2, 10, stop_tokens=[stop], penalty_range=3)
    first0 = free["top_tokens"].index(stop) if stop in free["top_tokens"] else None
    if first0 is None:
        assert r["tokens"] == free["tokens"]
    else:       # identical until hypothesis 0 itself takes it; then the loop ends with the stop token counted
        assert len(r["tokens"]) == first0 + 1 and r["tokens"][-1] == stop
        assert r["top_tokens"] == free["top_tokens"][: first0 + 1]
    # hypothesis 0's token at selection 4 as the stop id: the sentence ends at its first appearance on hypothesis 0
    stop0 = free["top_tokens"][4]
    k = free["top_tokens"].index(stop0)
    r0 = R.beam_generate(_Scripted(rows), None, 2, 10, stop_tokens=[stop0], penalty_range=3)
    assert len(r0["tokens"]) == k + 1 and r0["tokens"][-1] == stop0 and r0["hidden"].shape[0] == k + 1
    assert r0["pen"][stop0] == 1.0 or stop0 in r0["tokens"][:-1]                 # the stop token is not penalised


def test_max_new_limit():
    rows = _scripted_rows(12)
    for max_new in (0, 1, 2, 7):
        r = R.beam_generate(_Scripted(rows), None, 3, max_new)
        assert len(r["tokens"]) == max_new and r["hidden"].shape[0] == max_new and len(r["margins"]) == max_new


def test_unit_inputs_are_rarely_borderline():
    """the inputs of the GPU unit test: at most 1 % of the selections sit under the margin below which the device may differ"""
    n = low = 0
    for codes in R.UNIT_CODES:
        for groups in R.UNIT_GROUPS:
            for beams in R.UNIT_BEAMS:
                lg, pen, prev = R.unit_case(codes, groups, beams)
                for first in (True, False):
                    _, _, sc, margins = R.unit_reference(lg, pen, prev, groups, beams, first)
                    for g in range(groups):
                        n += 1
                        low += margins[g] < 4 * R.tol(sc[g]).max()
    assert n == 160 and low <= n // 100, (n, low)


def test_beams_keyword_checks():
    cfg0 = IndexGPTConfig.small()
    e = IndexGPT.__new__(IndexGPT)               # the checks come before anything touches the library or a device
    e.cfg = IndexGPTConfig(**{**cfg0.__dict__, "max_batch": 4})
    e._h = None
    p = np.zeros((1, 13, cfg0.hidden), np.float32)
    for call in (lambda **k: e.generate_from_prompt(p, 4, **k), lambda **k: e.generate_batch([p], [4], **k),
                 lambda **k: e.generate_batch_torch(None, [13], [4], None, None, **k),
                 lambda **k: e.generate_torch(None, 4, None, None, **k)):
        for bad in (dict(beams=0), dict(beams=-1), dict(beams=9), dict(beams=2.5), dict(beams=5),
                    dict(beams=2, sampling=Sampling())):
            with pytest.raises(ValueError):
                call(**bad)
    with pytest.raises(ValueError):
        e.generate_batch([p, p, p], [4, 4, 4], beams=2)             # 6 slots, max_batch 4
    with pytest.raises(ValueError):
        e.generate_beam([p], [4], 5)
