"""CPU: the float64 restatement of pool-mode beam search (tests/gpt_beam_pool_ref.py) against transformers' own beam search on a
tiny random GPT-2, its Gumbel-top-K draw against the Plackett-Luce distribution, one beam against the greedy reference, and the
argument errors of the host model (IndexGPT.generate_beam's checks that need no device)."""
import itertools

import numpy as np
import pytest

import gpt_beam_pool_ref as R
import gpt_beam_ref as RB

VOCAB = 40
MAX_NEW = 12


# ---------------------------------------------------------------------------------------------------------------
# against transformers
# ---------------------------------------------------------------------------------------------------------------
class _HFModel:
    """the reference's model protocol over a transformers causal LM: kv is the token list, every step a full forward"""

    def __init__(self, model):
        self.m = model

    def _logits(self, ids):
        import torch
        with torch.no_grad():
            return self.m(torch.tensor([ids])).logits[0, -1].float().numpy().copy()

    def prompt(self, prompt):
        ids = [int(t) for t in prompt]
        return self._logits(ids), np.zeros(1, np.float32), ids

    def step(self, kv, token, gen_len):
        ids = kv + [int(token)]
        return self._logits(ids), np.zeros(1, np.float32), ids


@pytest.fixture(scope="module")
def hf():
    pytest.importorskip("transformers")
    torch = pytest.importorskip("torch")
    from transformers import GPT2Config, GPT2LMHeadModel
    models = {}

    def get(seed, spread=0.6):
        """spread = the initialiser's standard deviation: 0.6 gives peaked rows, 0.2 rows on which top-p keeps many codes"""
        if (seed, spread) not in models:
            torch.manual_seed(seed)
            cfg = GPT2Config(vocab_size=VOCAB, n_positions=32, n_embd=16, n_layer=1, n_head=2, initializer_range=spread,
                             bos_token_id=0, eos_token_id=1)
            models[seed, spread] = GPT2LMHeadModel(cfg).eval()
        return models[seed, spread]
    return get


def _hf_generate(model, prompt, B, stops, lp, es, sampling=None, max_new=MAX_NEW):
    import torch
    kw = dict(num_beams=B, max_new_tokens=max_new, eos_token_id=list(stops), pad_token_id=VOCAB - 1, length_penalty=lp,
              early_stopping=es, return_dict_in_generate=True, output_scores=True, do_sample=sampling is not None)
    if sampling is not None:
        kw.update(top_k=sampling["top_k"], top_p=sampling["top_p"], temperature=sampling["temperature"])
    with torch.no_grad():
        out = model.generate(torch.tensor([prompt]), **kw)
    seq = out.sequences[0, len(prompt):].tolist()
    score = float(out.sequences_scores[0]) if getattr(out, "sequences_scores", None) is not None else None
    return seq, score


def _cases():
    for B, n_stop, lp, es in itertools.product((1, 2, 3, 4), (1, 2), (0.0, 1.0, -0.5), (False, True)):
        for seed in (1, 2):
            yield B, n_stop, lp, es, seed


_STOP_CACHE = {}


def _stops(model, prompt, n_stop):
    """stop ids a search is sure to meet: tokens 3 and 6 of the model's own greedy continuation"""
    key = (id(model), n_stop)
    if key not in _STOP_CACHE:
        g = R.pool_generate(_HFModel(model), prompt, 1, MAX_NEW, repeat_value=1.0)["tokens"]
        _STOP_CACHE[key] = tuple(dict.fromkeys((g[3], g[6])))[:n_stop] if n_stop == 2 else (g[3],)
    return _STOP_CACHE[key]


def _check(seq, score, ref, what):
    toks = ref["tokens"]
    assert seq[: len(toks)] == toks and all(t == VOCAB - 1 for t in seq[len(toks):]), (what, seq, toks)
    if score is not None:
        assert abs(score - ref["score"]) <= 1e-5, (what, score, ref["score"])


def test_deterministic_pool_vs_transformers(hf):
    n = low = early = pooled = limit = opened = 0
    for B, n_stop, lp, es, seed in _cases():
        model = hf(seed)
        prompt = [(3 * seed + 5 * k) % VOCAB for k in range(4)]
        stops = _stops(model, prompt, n_stop)
        ref = R.pool_generate(_HFModel(model), prompt, B, MAX_NEW, stop_tokens=stops, repeat_value=1.0,
                              length_penalty=lp, early_stopping=es)
        n += 1
        if min(ref["margins"]) < R.MARGIN:
            low += 1
            continue
        seq, score = _hf_generate(model, prompt, B, stops, lp, es)
        _check(seq, score, ref, (B, n_stop, lp, es, seed))
        early += len(ref["tokens"]) < MAX_NEW
        pooled += ref["from_pool_only"]
        limit += len(ref["tokens"]) == MAX_NEW
        opened += ref["ended_by_open"]
    print(f"pool vs transformers: {n} cases, {low} under the margin, {early} end before the limit, {pooled} decided by the pool, "
          f"{limit} run to the limit, {opened} ended by `open`")
    assert n == 96 and low * 10 <= n
    assert early >= 1 and pooled >= 1 and limit >= 1 and opened >= 1


def test_sampled_pool_vs_transformers(hf, monkeypatch):
    """do_sample=True with torch.multinomial replaced by the definition's draw: ordering by log(probs) + the Gumbel noise of
    that call's selection index.  The warp order, the pool and the stop rule around the draw are transformers' own."""
    import torch
    state = {}

    def draw(probs, num_samples, **kw):
        p = probs[0].double().numpy()
        idx = np.flatnonzero(p > 0)
        key = np.full(p.shape, -np.inf)
        key[idx] = np.log(p[idx]) + R.gumbel(state["seed"], state["n"], idx)
        state["n"] += 1
        return torch.tensor(np.argsort(-key, kind="stable")[:num_samples].copy())[None]

    monkeypatch.setattr(torch, "multinomial", draw)
    n = low = forced = early = 0
    # The deterministic run's cases without B = 1 (transformers does no beam sampling at num_beams = 1) and without
    # length_penalty -0.5: drawn hypotheses are unlikely ones, their scores times sqrt(length) reach -75 to -130, and transformers
    # accumulates its score in fp32, whose one to two ulps there (0.8e-5 to 1.5e-5) are what the 1e-5 bound would then measure.
    for B, n_stop, lp, es in itertools.product((2, 3, 4), (1, 2), (0.0, 1.0), (False, True)):
        for seed, (T, tk, tp) in ((1, (1.0, 30, 0.8)), (2, (1.25, 0, 0.9)), (3, (0.8, 20, 1.0))):
            model = hf(seed, 0.2)
            prompt = [(3 * seed + 5 * k) % VOCAB for k in range(4)]
            sp = dict(temperature=T, top_k=tk, top_p=tp, seed=1000 + seed)
            stops = _stops(model, prompt, n_stop)
            ref = R.pool_generate(_HFModel(model), prompt, B, MAX_NEW, stop_tokens=stops, repeat_value=1.0,
                                  length_penalty=lp, early_stopping=es, sampling=sp)
            n += 1
            if ref["forced"]:                                   # min_tokens_to_keep = K decided: transformers keeps n_stop + 1
                forced += 1
                continue
            if min(ref["margins"]) < R.MARGIN:
                low += 1
                continue
            state.update(seed=sp["seed"], n=0)
            seq, score = _hf_generate(model, prompt, B, stops, lp, es, sp)
            _check(seq, score, ref, (B, n_stop, lp, es, seed))
            early += len(ref["tokens"]) < MAX_NEW
    print(f"sampled pool vs transformers: {n} cases, {low} under the margin, {forced} outside transformers' own rule, "
          f"{early} end before the limit")
    assert n == 72 and low * 10 <= n and forced * 10 <= n and early >= 1


# ---------------------------------------------------------------------------------------------------------------
# the draw, one beam, argument errors
# ---------------------------------------------------------------------------------------------------------------
def test_gumbel_top_k_is_sampling_without_replacement():
    """6 candidates, 20 000 seeds: the first draw and the ordered first pair within 5 binomial standard deviations of
    Plackett-Luce (p_a, and p_a * p_b / (1 - p_a))"""
    p = np.array([0.35, 0.25, 0.15, 0.12, 0.08, 0.05])
    acc = np.log(p) - 1.7
    N = 20000
    first = np.zeros(6)
    pair = np.zeros((6, 6))
    idx = np.arange(6)
    for seed in range(N):
        order = np.argsort(-(acc + R.gumbel(seed, 3, idx)), kind="stable")
        first[order[0]] += 1
        pair[order[0], order[1]] += 1
    for a in range(6):
        assert abs(first[a] - N * p[a]) <= 5 * np.sqrt(N * p[a] * (1 - p[a])), (a, first[a])
        for b in range(6):
            if a != b:
                q = p[a] * p[b] / (1 - p[a])
                assert abs(pair[a, b] - N * q) <= 5 * np.sqrt(N * q * (1 - q)), (a, b, pair[a, b])


class _TableModel:
    """logits from a fixed random table by (last token, position): enough of a model for loops that only need logits"""

    def __init__(self, codes, seed):
        self.t = (3.0 * np.random.default_rng(seed).standard_normal((codes + 1, 40, codes))).astype(np.float32)

    def prompt(self, prompt):
        return self.t[-1, 0], np.zeros(2, np.float32), None

    def step(self, kv, token, gen_len):
        return self.t[token, gen_len], np.full(2, gen_len, np.float32), None


def test_one_beam_is_the_greedy_reference():
    for seed in range(6):
        m = _TableModel(50, seed)
        stops = (7, 11)
        g = RB.beam_generate(m, None, 1, 20, stop_tokens=stops, repeat_value=0.7, penalty_range=3)
        r = R.pool_generate(m, None, 1, 20, stop_tokens=stops, repeat_value=0.7, penalty_range=3)
        assert r["tokens"] == g["tokens"] and abs(r["score"] - g["score"]) <= R.tol(g["score"])
        np.testing.assert_array_equal(r["hidden"], g["hidden"])


def test_select_keeps_an_old_entry_over_an_equal_new_one():
    lg = np.zeros((2, 8), np.float32)
    lg[:, 3] = 5.0                                              # both rows finish with code 3 at the same acc
    r0 = R.select(lg, None, [-1.0, -1.0], 2, 9, [3], 2, [R.NEG, R.NEG], [False, False], True)
    assert r0["pool_src"] == [("new", 0), ("new", 1)] and r0["pool_fin"].all()
    r1 = R.select(lg, None, [-1.0, -1.0], 3, 9, [3], 2, r0["pool_score"], r0["pool_fin"], True)
    assert r1["pool_src"] == [("old", 0), ("old", 1)] and not r1["open"] and r1["done"]


def test_unit_cases_are_mostly_decided():
    """the unit cases of tests/test_gpu_gpt_beam_pool.py: at most 5 % may fall under the margin, by the reference alone"""
    n = low = forced = 0
    for codes in R.unit_codes():
        for beams in R.UNIT_BEAMS:
            for n_stop in R.UNIT_NSTOP:
                K = (n_stop + 1) * beams
                if K > 64 or (codes != "K" and K > codes):
                    continue
                for first in (True, False):
                    for sampled in (False, True):
                        r = R.select(**R.unit_case(codes, beams, n_stop, first, sampled))
                        n += 1
                        low += r["margin"] < R.MARGIN
                        forced += r["forced"]
    print(f"unit cases: {n}, {low} under the margin, {forced} keep a code by the K-best rule")
    assert n == 296 and low * 20 <= n and forced >= 10


def test_sampled_tie_cases_reach_the_k_best_rule():
    """the sampled tie cases of the GPU test: top-p leaves fewer than K codes, the K best rule decides, and in most of them equal
    values lie across the K-th place; the kept set is then the K lowest-index best codes of every row"""
    n = across = 0
    for beams in R.UNIT_BEAMS:
        for n_stop in (0, 1, 3):
            for first in (True, False):
                kw = R.tie_case_sampled(beams, n_stop, first)
                r = R.select(**kw)
                K = (n_stop + 1) * beams
                rows = 1 if first else beams
                row = np.asarray(kw["logits"], np.float64)[0]
                want = np.sort(np.argsort(-row, kind="stable")[:K])
                assert (r["forced"] or K == 1) and r["kept"].reshape(rows, -1).sum(axis=1).tolist() == [K] * rows
                for b in range(rows):
                    assert np.flatnonzero(r["kept"].reshape(rows, -1)[b]).tolist() == want.tolist()
                n += 1
                across += R.ties_across_kth(kw)
    assert n == 30 and across >= 15, (n, across)


def test_host_argument_errors():
    from mi355tts.config import IndexGPTConfig
    from mi355tts.indextts import Sampling, _check_beams
    cfg = IndexGPTConfig(**{**IndexGPTConfig.small().__dict__, "max_batch": 8})
    sp = [Sampling(1.0, 30, 0.8, 1)]
    with pytest.raises(ValueError):
        _check_beams(3, 1, cfg, sampling=sp)                    # sampling needs pool=True
    assert _check_beams(3, 1, cfg, sampling=sp, pool=True) == 3
    assert _check_beams(1, 1, cfg, sampling=sp) == 1
    for bad in (0, 9, 2.5, True):
        with pytest.raises(ValueError):
            _check_beams(bad, 1, cfg, pool=True)
    with pytest.raises(ValueError):
        _check_beams(3, 3, cfg, pool=True)                      # 9 slots, the engine has 8
