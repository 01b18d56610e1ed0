"""Float64 restatement of pool-mode beam search (include/mi355tts.h, "beam search with a finished pool"): TEST INFRASTRUCTURE.

``select`` is one selection with the whole state passed in and out; ``pool_generate`` is the definition's loop over any model that
gives logits (the model classes of tests/gpt_beam_ref.py).  Every hypothesis and every pool entry owns a full copy of its
history, which is what the device's ancestor tables and frozen lists have to be indistinguishable from.

Every result carries a margin: how far the selection is from a decision that fp32 rounding could flip (membership and order of
the K candidates, the running hypotheses, the pool merge, the `open` test, and in sampling mode the top-k / top-p thresholds).
A test compares wherever the margin is at least MARGIN and leaves the case undecided elsewhere."""
from __future__ import annotations

import numpy as np

from gpt_sampling_ref import MASK, philox4x32_10

NEG = -1.0e9              # score of a pool entry that holds nothing yet
MARGIN = 1e-4
TOL_ABS = 1e-5            # tests/gpt_beam_ref.py's bound for a score
TOL_REL = 2.0 ** -22
Z_TIE = 1e-5              # two values of a row closer than this may round to one fp32 value after z - lse and * inv_T
P_BAND = 1e-5             # relative band around top_p * S inside which the device's integer masses may decide otherwise


def tol(score):
    return TOL_ABS + TOL_REL * np.abs(score)


def _philox_words(seed, n, blocks):
    """Philox4x32-10 of gpt_sampling_ref.philox4x32_10 over an array of counters (n, block, 1, 0): (len(blocks), 4) words"""
    from gpt_sampling_ref import M0, M1, W0, W1
    c = [np.full(blocks.shape, int(n) & MASK, np.uint64), blocks.astype(np.uint64), np.ones(blocks.shape, np.uint64),
         np.zeros(blocks.shape, np.uint64)]
    k0, k1 = int(seed) & MASK, (int(seed) >> 32) & MASK
    m = np.uint64(MASK)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(c, axis=-1)


def gumbel(seed, n, idx):
    """g(i) of step 4 for flat indices idx: -log(-log u), u = ((word >> 8) + 0.5) * 2^-24, word = output (i & 3) of Philox4x32-10
    with counter (n, i >> 2, 1, 0) and the seed as key"""
    idx = np.asarray(idx, np.int64).reshape(-1)
    if idx.size == 0:
        return np.zeros(0)
    blocks, inv = np.unique(idx >> 2, return_inverse=True)
    words = _philox_words(seed, n, blocks)[inv, idx & 3]
    u = ((words >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    return -np.log(-np.log(u))


def warp_row(lp, temperature, top_k, top_p, keep):
    """Step 2 in sampling mode on one row of log-probabilities (float64): w = lp * inv_T, top-k and top-p by the sampler's steps
    2-4 applied to w, the `keep` best codes always kept.  Returns (w, forced, amb): forced = the `keep` rule added a code that
    top-k / top-p had left out; amb = bool mask of the codes whose membership rounding may decide (None when the top-k threshold
    itself is undecided: margin 0)."""
    codes = lp.size
    inv_t = float(np.float32(1.0) / np.float32(temperature))
    w = lp * inv_t
    order = np.argsort(-w, kind="stable")
    forced = np.zeros(codes, bool)
    forced[order[:keep]] = True
    undecided = False
    if 0 < top_k < codes:
        t_k = w[order[top_k - 1]]
        K = w >= t_k
        nxt = w[order[top_k]]
        undecided = 0.0 < t_k - nxt < Z_TIE
    else:
        K = np.ones(codes, bool)
    e = np.where(K, np.exp(w - w.max()), 0.0)
    S = e.sum()
    amb = np.zeros(codes, bool)
    tp = float(np.float32(top_p))
    if tp >= 1.0:
        P = K.copy()
    else:
        kidx = np.flatnonzero(K)
        ko = kidx[np.argsort(-w[kidx], kind="stable")]
        ws, cs = w[ko], np.cumsum(e[ko])
        ends = np.flatnonzero(np.append(ws[1:] != ws[:-1], True))
        vals, cum = ws[ends], cs[ends]
        target = tp * S
        hit = cum >= target
        i = int(np.argmax(hit)) if hit.any() else len(vals) - 1
        P = K & (w >= vals[i])
        below = cum[i - 1] if i > 0 else 0.0
        if target - below < P_BAND * target:                       # the group at the threshold may be left out
            amb |= K & (w == vals[i])
        if cum[i] - target < P_BAND * target and i + 1 < len(vals):   # the next group may be taken in
            amb |= K & (w == vals[i + 1])
        amb |= K & ~P & (w > vals[i] - Z_TIE)                       # may round to the threshold's fp32 value
    kept = P | forced
    amb &= ~forced
    return np.where(kept | amb, w, -np.inf), bool((forced & ~P).any()), (None if undecided else amb)


def _gaps(vals):
    v = np.asarray(vals, np.float64)
    v = v[np.isfinite(v)]
    return float(np.min(v[:-1] - v[1:])) if len(v) > 1 else float("inf")


def select(logits, pen, scores, n, max_new, stops, beams, pool_score, pool_fin, open_, length_penalty=0.0, early_stopping=False,
           sampling=None):
    """One selection.  logits (beams, codes) float32 (n == 0: only row 0 is read), pen likewise or None, scores (beams,) running
    scores (ignored at n == 0), pool_score / pool_fin (beams,), open_ bool, sampling None or dict(temperature, top_k, top_p, seed).
    Returns a dict:
      cand, cand_acc, cand_stop   the K candidates in candidate order: flat index, acc, stop flag
      run                         positions (into cand) of the next running hypotheses; parents, tokens, scores follow them
      pool_score, pool_fin        the pool after the merge; pool_src[j] = ("old", j') or ("new", position into cand)
      kept                        (R * codes,) bool: the flat indices step 2 left in (all of them in deterministic mode)
      open, done, margin; forced: sampling mode kept a code only because the K best of a row always stay"""
    lg = np.asarray(logits, np.float32)
    B = int(beams)
    pn = np.ones_like(lg) if pen is None else np.asarray(pen, np.float32)
    z = (lg * pn).astype(np.float32)
    first = n == 0
    if first:
        z = z[:1]
    R, codes = z.shape
    stops = [int(s) for s in stops]
    K = (len(stops) + 1) * B
    zz = z.astype(np.float64)
    m = zz.max(axis=1, keepdims=True)
    lp = zz - (m + np.log(np.exp(zz - m).sum(axis=1, keepdims=True)))
    margin = float("inf")
    forced = False
    amb = np.zeros((R, codes), bool)
    if sampling is None:
        w = lp
    else:
        w = np.empty_like(lp)
        for b in range(R):
            w[b], f, a = warp_row(lp[b], sampling["temperature"], int(sampling["top_k"]), sampling["top_p"], K)
            forced |= f
            if a is None:
                margin = 0.0
            else:
                amb[b] = a
    base = np.zeros((R, 1)) if first else np.asarray(scores, np.float32).astype(np.float64).reshape(-1, 1)
    acc = (base + w).reshape(-1)
    if sampling is None:
        key = acc
    else:
        key = np.full(acc.shape, -np.inf)
        fin = np.flatnonzero(np.isfinite(acc))
        key[fin] = acc[fin] + gumbel(sampling["seed"], n, fin)
    order = np.argsort(-key, kind="stable")[: K + 1]
    if amb.reshape(-1)[order].any():
        margin = 0.0
    margin = min(margin, _gaps(key[order]))
    cand = order[:K]
    cand_acc = acc[cand]
    last = n + 1 == max_new
    cand_stop = np.array([last or int(i % codes) in stops for i in cand], bool)
    # next running hypotheses: the B candidates of largest acc among those that do not stop, ties to the earlier candidate
    live = np.flatnonzero(~cand_stop)
    lo = live[np.argsort(-cand_acc[live], kind="stable")]
    run = lo[:B]
    if sampling is not None:
        margin = min(margin, _gaps(cand_acc[lo[: B + 1]]))
    new_scores = cand_acc[run]
    # pool
    pool_score = np.asarray(pool_score, np.float64).copy()
    pool_fin = np.asarray(pool_fin, bool).copy()
    scale = float(n + 1) ** float(length_penalty)
    items = [(pool_score[j], bool(pool_fin[j]), ("old", j)) for j in range(B)]
    if open_ and not (early_stopping and pool_fin.all()):
        for q in range(min(B, K)):
            if cand_stop[q]:
                items.append((cand_acc[q] / scale, True, ("new", int(q))))
    idx = sorted(range(len(items)), key=lambda t: -items[t][0])    # stable: old before new, then candidate order
    sv = [items[t][0] for t in idx[: B + 1]]
    for a in range(len(sv) - 1):
        if items[idx[a]][2][0] == "new" or items[idx[a + 1]][2][0] == "new":
            margin = min(margin, sv[a] - sv[a + 1])
    keep = idx[:B]
    pool_score = np.array([items[t][0] for t in keep])
    pool_fin = np.array([items[t][1] for t in keep], bool)
    pool_src = [items[t][2] for t in keep]
    if pool_fin.all() and len(run):
        best = new_scores[0] / scale
        margin = min(margin, abs(best - pool_score.min()))
        open_ = bool(open_ and best > pool_score.min())
    done = (not open_) or (early_stopping and bool(pool_fin.all())) or last
    return dict(cand=cand.astype(np.int64), cand_acc=cand_acc, cand_stop=cand_stop, run=run,
                parents=(cand[run] // codes).astype(np.int32), tokens=(cand[run] % codes).astype(np.int32), scores=new_scores,
                pool_score=pool_score, pool_fin=pool_fin, pool_src=pool_src, open=bool(open_), done=bool(done), margin=float(margin), forced=forced, kept=np.isfinite(acc))


class _Hyp:
    __slots__ = ("tokens", "hid", "pen", "reset", "kv", "score")

    def __init__(self, tokens, hid, pen, reset, kv, score):
        self.tokens, self.hid, self.pen, self.reset, self.kv, self.score = tokens, hid, pen, reset, kv, score


def _bookkeeping(h, t, repeat_value, penalty_range):
    """the greedy loop's penalty bookkeeping for the token just appended; a running hypothesis never holds a stop id"""
    h.pen[t] = repeat_value
    if len(h.tokens) > penalty_range and h.tokens[h.reset] != t:
        h.pen[h.tokens[h.reset]] = 1.0
        h.reset += 1


def pool_generate(model, prompt, beams, max_new, *, stop_tokens=(), repeat_value=0.7, penalty_range=3, pen0=None,
                  length_penalty=0.0, early_stopping=False, sampling=None):
    """The definition's loop (models: tests/gpt_beam_ref.py).  Running scores are carried as float32 values, every selection is
    evaluated in float64.  Returns dict(tokens, hidden (n, hidden), score, margins (one per selection), from_pool_only: the
    returned entry is not candidate 0 of the last selection (the one hypothesis the search without a pool could return),
    forced: some selection kept a code only by the K-best rule (where transformers, keeping n_stop + 1, would differ),
    zmax: the largest |logits * pen| any selection read, ended_by_open: `open` went false before any limit)."""
    stops = [int(s) for s in stop_tokens]
    rv = np.float32(repeat_value)
    B = int(beams)
    out = {"margins": [], "forced": False, "zmax": 0.0}
    if max_new <= 0:
        out.update(tokens=[], hidden=None, score=0.0, from_pool_only=False, ended_by_open=False)
        return out
    logits, last, kv = model.prompt(prompt)
    codes = logits.shape[-1]
    pen0 = np.ones((codes,), np.float32) if pen0 is None else np.asarray(pen0, np.float32).reshape(-1).copy()
    pool_score, pool_fin, open_ = np.full(B, NEG), np.zeros(B, bool), True
    pool = [None] * B
    hyps = [_Hyp([], [], pen0, 0, kv, np.float32(0.0))]
    res = [(logits, last, kv)]
    n = 0
    while True:
        L = np.stack([res[min(b, len(res) - 1)][0] for b in range(B)])
        P = np.stack([hyps[min(b, len(hyps) - 1)].pen for b in range(B)])
        r = select(L, P, [h.score for h in hyps] + [0.0] * (B - len(hyps)), n, max_new, stops, B, pool_score, pool_fin, open_,
                   length_penalty, early_stopping, sampling)
        out["margins"].append(r["margin"])
        out["forced"] |= r["forced"]
        out["zmax"] = max(out["zmax"], float(np.abs(L[: len(res)] * P[: len(res)]).max()))

        def child(q):
            i = int(r["cand"][q])
            p, t = i // codes, i % codes
            return hyps[p], res[p], t

        new_pool = []
        for j, (kind, src) in enumerate(r["pool_src"]):
            if kind == "old":
                new_pool.append(pool[src])
            else:
                h, rs, t = child(src)
                new_pool.append(dict(tokens=h.tokens + [t], hid=h.hid + [rs[1]], score=float(r["pool_score"][j]), at=(n, int(src))))
        pool, pool_score, pool_fin, open_ = new_pool, r["pool_score"], r["pool_fin"], r["open"]
        new = []
        for k, q in enumerate(r["run"]):
            h, rs, t = child(int(q))
            c = _Hyp(h.tokens + [t], h.hid + [rs[1]], h.pen.copy(), h.reset, rs[2], np.float32(r["scores"][k]))
            _bookkeeping(c, t, rv, penalty_range)
            new.append(c)
        if r["done"]:
            break
        hyps = new
        n += 1
        res = [model.step(h.kv, h.tokens[-1], n) for h in hyps]
    best = pool[0]
    out.update(tokens=best["tokens"], hidden=np.stack(best["hid"]).astype(np.float32), score=best["score"],
               from_pool_only=best["at"] != (n, 0),
               ended_by_open=(not open_) and n + 1 < max_new and not (early_stopping and bool(pool_fin.all())))
    return out


# ---- inputs of the unit entry's tests ---------------------------------------------------------------------------------------------
UNIT_BEAMS = (1, 2, 3, 5, 8)
UNIT_NSTOP = (0, 1, 6)
UNIT_SEED = 9527


def unit_codes():
    """the code counts of the unit cases: "K" stands for K itself (every code is a candidate at selection 0)"""
    return ("K", 37, 1030, 8194, 16384)


def unit_case(codes, beams, n_stop, first, sampled, seed=UNIT_SEED):
    """logits 3 * N(0, 1), a fifth of the penalties off 1, previous scores around -5; stop ids among the likeliest codes of the
    rows (so that candidates do stop); at n >= 1 a pool whose first half is finished with scores around the running ones.
    Returns the keyword arguments of select() / beam_pool_select() that both take."""
    K = (n_stop + 1) * beams
    codes = K if codes == "K" else int(codes)
    rng = np.random.default_rng([seed, codes, beams, n_stop, int(first), int(sampled)])
    lg = (3.0 * rng.standard_normal((beams, codes))).astype(np.float32)
    u = rng.random((beams, codes))
    pen = np.where(u < 0.1, 0.7, np.where(u > 0.9, 1.3, 1.0)).astype(np.float32)
    prev = (-5.0 + rng.standard_normal(beams)).astype(np.float32)
    zz = lg * pen
    top = np.argsort(-(zz[0] if first else zz.max(axis=0)), kind="stable")
    stops = [int(t) for t in top[1: 2 * n_stop: 2]]
    n = 0 if first else 5
    max_new = 6 if (n_stop == 6 and not first) else 40                 # some cases sit at the limit: every candidate stops
    if first:
        ps, pf = np.full(beams, NEG, np.float32), np.zeros(beams, bool)
    else:
        h = (beams + 1) // 2
        ps = np.concatenate([np.sort(-6.0 - rng.random(h))[::-1], np.full(beams - h, NEG)]).astype(np.float32)
        pf = np.arange(beams) < h
        if beams % 2:                                                  # odd beam counts start with a full pool
            ps = np.sort(-6.0 - 2.0 * rng.random(beams))[::-1].astype(np.float32)
            pf = np.ones(beams, bool)
    sp = None
    if sampled:
        sp = [dict(temperature=1.0, top_k=max(30, K), top_p=0.8, seed=seed + codes), dict(temperature=0.7, top_k=0, top_p=1.0, seed=11),
              dict(temperature=1.3, top_k=0, top_p=0.6, seed=2 ** 40 + 5)][(beams + n_stop) % 3]
    return dict(logits=lg, pen=pen, scores=prev, n=n, max_new=max_new, stops=stops, beams=beams, pool_score=ps, pool_fin=pf,
                open_=True, length_penalty=(0.0, 1.0)[beams % 2], early_stopping=bool(n_stop == 1), sampling=sp)


def tie_case(beams, n_stop, first, codes=64, seed=4):
    """`beams` identical rows of logits in steps of 0.25 and equal previous scores: exact ties inside and across rows, stop ids
    among the tied codes"""
    rng = np.random.default_rng(seed)
    row = (np.round(rng.standard_normal(codes) * 4.0) / 4.0).astype(np.float32)
    top = np.argsort(-row, kind="stable")
    return dict(logits=np.tile(row, (beams, 1)), pen=None, scores=np.full(beams, -3.5, np.float32), n=0 if first else 3, max_new=40,
                stops=[int(t) for t in top[1: 1 + n_stop]], beams=beams, pool_score=np.full(beams, NEG, np.float32),
                pool_fin=np.zeros(beams, bool), open_=True, length_penalty=0.0, early_stopping=False, sampling=None)


def tie_case_sampled(beams, n_stop, first, codes=64, seed=4):
    """tie_case in sampling mode with a top_p so small that P holds fewer than K codes: every row keeps exactly its K best, and
    the steps of 0.25 put equal values across the K-th place, which go to the lower code"""
    kw = tie_case(beams, n_stop, first, codes, seed)
    kw["sampling"] = dict(temperature=1.0, top_k=0, top_p=0.05, seed=77 + beams)
    return kw


def ties_across_kth(kw):
    """True when row 0 of the case has equal values at places K and K + 1 of its descending order"""
    K = (len(kw["stops"]) + 1) * kw["beams"]
    v = np.sort(np.asarray(kw["logits"], np.float64)[0])[::-1]
    return K < v.size and v[K - 1] == v[K]
