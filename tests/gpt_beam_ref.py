"""Float64 restatement of the beam search definition in include/mi355tts.h ("beam search"): TEST INFRASTRUCTURE.

``select`` is one selection on rows of logits; ``beam_generate`` is the whole loop over any model that gives logits — the numpy
oracle with per-hypothesis copies of keys and values (``OracleModel``) or the engine's own single-sentence step with the cache
swapped per hypothesis (``EngineModel``).  Neither knows about slots, ancestor tables or shared caches: every hypothesis owns
a full copy of everything, which is what the device code has to be indistinguishable from."""
from __future__ import annotations

import numpy as np

TOL_ABS = 1e-5            # the project's tolerance for softmax-derived quantities (the sampler tests)
TOL_REL = 2.0 ** -22      # a few fp32 roundings of the stored sum


def tol(score):
    return TOL_ABS + TOL_REL * np.abs(score)


def select(logits, pen, prev, beams, first):
    """logits (beams, codes) float32 (first: only row 0 is read), pen likewise or None, prev (beams,) or None when first.
    Returns parents (beams,), tokens (beams,), scores (beams,) float64 and the margin: the smallest gap between consecutive
    entries of the sorted top beams + 1 candidates (it decides membership and order; inf when there is no runner-up)."""
    lg = np.asarray(logits, np.float32)
    pn = np.ones_like(lg) if pen is None else np.asarray(pen, np.float32)
    z = (lg * pn).astype(np.float32)                              # one fp32 multiply
    if first:
        z = z[:1]
    codes = z.shape[1]
    zz = z.astype(np.float64)
    m = zz.max(axis=1, keepdims=True)
    lse = m + np.log(np.exp(zz - m).sum(axis=1, keepdims=True))
    cand = zz - lse
    if not first:
        cand = np.asarray(prev, np.float64).reshape(-1, 1) + cand
    flat = cand.reshape(-1)
    order = np.argsort(-flat, kind="stable")                     # descending; a tie goes to the lower flat index
    top = order[: beams + 1]
    vals = flat[top]
    margin = float(np.min(vals[:-1] - vals[1:])) if len(vals) > 1 else float("inf")
    best = top[:beams]
    return (best // codes).astype(np.int32), (best % codes).astype(np.int32), flat[best].copy(), margin


class _Hyp:
    __slots__ = ("tokens", "hid", "pen", "reset", "kv", "score")

    def __init__(self, tokens, hid, pen, reset, kv, score):
        self.tokens, self.hid, self.pen, self.reset, self.kv, self.score = tokens, hid, pen, reset, kv, score


def _bookkeeping(h, t, is0, stops, repeat_value, penalty_range):
    """the greedy loop's bookkeeping for the token just appended (oracle/gpt_np.generate); only hypothesis 0 has a stop test"""
    if is0 and t in stops:
        return
    h.pen[t] = repeat_value
    if len(h.tokens) > penalty_range and h.tokens[h.reset] != t:
        h.pen[h.tokens[h.reset]] = 1.0
        h.reset += 1


def beam_generate(model, prompt, beams, max_new, *, stop_tokens=(), repeat_value=0.7, penalty_range=3, pen0=None):
    """The definition's loop.  ``model.prompt(prompt) -> (logits, last, kv)``, ``model.step(kv, token, gen_len) -> (logits,
    last, kv)``, logits before the penalty.  Scores are carried as float32 values (the definition's) and every selection is
    evaluated in float64.  Returns a dict: tokens, hidden (n, hidden), score, pen of hypothesis 0; margins (one per selection);
    top_tokens (hypothesis 0's token after every selection)."""
    stops = set(int(s) for s in stop_tokens)
    rv = np.float32(repeat_value)
    logits, last, kv = model.prompt(prompt)
    codes = logits.shape[-1]
    pen0 = np.ones((codes,), np.float32) if pen0 is None else np.asarray(pen0, np.float32).reshape(-1).copy()
    out = {"margins": [], "top_tokens": []}
    if max_new <= 0:
        out.update(tokens=[], hidden=np.zeros((0, last.shape[-1]), np.float32), score=0.0, pen=pen0)
        return out
    par, tok, sc, mg = select(logits[None], pen0[None], None, beams, True)
    out["margins"].append(mg)
    hyps = []
    for i in range(beams):
        h = _Hyp([int(tok[i])], [last], pen0.copy(), 0, kv, np.float32(sc[i]))
        _bookkeeping(h, int(tok[i]), i == 0, stops, rv, penalty_range)
        hyps.append(h)
    n = 0
    while True:
        out["top_tokens"].append(hyps[0].tokens[-1])
        if hyps[0].tokens[-1] in stops or n + 1 == max_new:
            break
        n += 1
        res = [model.step(h.kv, h.tokens[-1], n) for h in hyps]
        L = np.stack([r[0] for r in res])
        par, tok, sc, mg = select(L, np.stack([h.pen for h in hyps]), np.array([h.score for h in hyps]), beams, False)
        out["margins"].append(mg)
        new = []
        for i in range(beams):
            p, t = hyps[int(par[i])], int(tok[i])
            h = _Hyp(p.tokens + [t], p.hid + [res[int(par[i])][1]], p.pen.copy(), p.reset, res[int(par[i])][2], np.float32(sc[i]))
            _bookkeeping(h, t, i == 0, stops, rv, penalty_range)
            new.append(h)
        hyps = new
    b = hyps[0]
    out.update(tokens=b.tokens, hidden=np.stack(b.hid).astype(np.float32), score=float(b.score), pen=b.pen)
    return out


class OracleModel:
    """oracle.gpt_np graphs C and E; a hypothesis' kv is its own (keys, values, history) copy"""

    def __init__(self, cfg, st):
        from oracle import gpt_np as O
        self.O, self.cfg, self.st = O, cfg, st
        self.folds = [O.fold_layer(cfg, st, i) for i in range(cfg.layers)]
        self.ones = np.ones((1, cfg.mel_codes), np.float32)

    def prompt(self, prompt):
        c = self.cfg
        keys = [np.zeros((c.heads, c.head_dim, 0), np.float32)] * c.layers
        vals = [np.zeros((c.heads, 0, c.head_dim), np.float32)] * c.layers
        p = np.asarray(prompt, np.float32)
        keys, vals, kvl, last, _, lg = self.O.graph_e(c, self.st, keys, vals, 0, self.ones, p.shape[1], p, 1, self.folds)
        return lg[0], last[0], (keys, vals, int(kvl[0]))

    def step(self, kv, token, gen_len):
        hs, _ = self.O.graph_c(self.cfg, self.st, [[int(token)]], [int(gen_len)])
        keys, vals, kvl, last, _, lg = self.O.graph_e(self.cfg, self.st, kv[0], kv[1], kv[2], self.ones, 1, hs, 0, self.folds)
        return lg[0], last[0], (keys, vals, int(kvl[0]))


class EngineModel:
    """the engine's own single-sentence step (IndexGPT.step), the handle's cache swapped per hypothesis with kv_read / kv_write"""

    def __init__(self, eng):
        self.e = eng
        self.ones = np.ones((1, eng.cfg.mel_codes), np.float32)

    def _kv(self):
        kv = [self.e.kv_read(i) for i in range(self.e.cfg.layers)]
        return [k for k, _ in kv], [v for _, v in kv]

    def prompt(self, prompt):
        self.e.reset()
        _, last, _, lg = self.e.step(prompt, self.ones, attention_mask=1, return_logits=True)
        return lg[0].copy(), last[0].copy(), self._kv()

    def step(self, kv, token, gen_len):
        self.e.kv_write(kv[0], kv[1])
        hs, _ = self.e.mel_embed(int(token), int(gen_len))
        _, last, _, lg = self.e.step(hs, self.ones, attention_mask=0, return_logits=True)
        return lg[0].copy(), last[0].copy(), self._kv()


# ---- inputs of the unit entry's tests -----------------------------------------------------------------------------------------
UNIT_CODES = (50, 1000, 8194, 16384)
UNIT_GROUPS = (1, 3)
UNIT_BEAMS = (1, 2, 3, 5, 8)


def unit_case(codes, groups, beams, seed=9527):
    """logits 3 * N(0, 1), penalties around 1 (a tenth of them 0.7, a tenth 1.3), previous scores in [-40, 0]"""
    rng = np.random.default_rng([seed, codes, groups, beams])
    rows = groups * beams
    lg = (3.0 * rng.standard_normal((rows, codes))).astype(np.float32)
    u = rng.random((rows, codes))
    pen = np.where(u < 0.1, 0.7, np.where(u > 0.9, 1.3, 1.0)).astype(np.float32)
    prev = (-40.0 * rng.random(rows)).astype(np.float32)
    return lg, pen, prev


def unit_reference(lg, pen, prev, groups, beams, first):
    """select() per group -> parents, tokens, scores (groups, beams) and margins (groups,)"""
    out = [select(lg[g * beams:(g + 1) * beams], pen[g * beams:(g + 1) * beams], prev[g * beams:(g + 1) * beams], beams, first)
           for g in range(groups)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]),
            np.array([o[3] for o in out]))


def tie_rows(beams, codes=64, seed=4):
    """`beams` identical rows of logits in steps of 0.25 (exact ties inside and across rows), equal previous scores"""
    rng = np.random.default_rng(seed)
    row = (np.round(rng.standard_normal(codes) * 4.0) / 4.0).astype(np.float32)
    return np.tile(row, (beams, 1)), np.full((beams,), -3.5, np.float32)
