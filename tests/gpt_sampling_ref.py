"""Float64 restatement of the IndexTTS GPT sampling definition (include/mi355tts.h, "sampling"), for the tests.

Philox4x32-10 in numpy integer arithmetic; z in float32 exactly as the header states it (two multiplies, no add: bit-equal to
the device); the sets K and P, the probabilities and the index-order CDF in float64.  ``sample`` also returns a margin: how
far the case is from a decision that rounding could flip, so that a test can leave token equality undecided on a borderline
case and on nothing else.
"""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: 4 uint32 words, key: 2 uint32 words -> the 4 output words (Salmon et al., SC'11; Random123 philox4x32-10)."""
    c = [int(x) & MASK for x in counter]
    k = [int(x) & MASK for x in key]
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> 32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return c


def uniform(seed: int, n: int) -> np.float32:
    """u of step 5 for decode index n: (w0 >> 8) * 2^-24, exact in float32"""
    w0 = philox4x32_10((n & MASK, (n >> 32) & MASK, 0, 0), (seed & MASK, (seed >> 32) & MASK))[0]
    return np.float32((w0 >> 8) * 2.0 ** -24)


def z32(logits, pen, temperature) -> np.ndarray:
    """step 1 in float32: (logits * pen) * inv_T, inv_T = 1.0f / temperature"""
    lg = np.asarray(logits, np.float32)
    pn = np.ones_like(lg) if pen is None else np.asarray(pen, np.float32)
    inv_t = np.float32(1.0) / np.float32(temperature)
    return ((lg * pn).astype(np.float32) * inv_t).astype(np.float32)


def sample(logits, pen, temperature, top_k, top_p, seed, n):
    """One row.  Returns a dict: token, u (float32), K and P (bool masks), probs (float64: e / S_P on P, 0 elsewhere) and margin
    = min(relative distance of top_p * S from the two cumulative masses that bracket t_p, distance of u from the nearest edge of
    the index-order CDF); inf where no rounding can matter (greedy)."""
    lg = np.asarray(logits, np.float32).reshape(-1)
    codes = lg.size
    u = uniform(int(seed), int(n))
    if top_k == 1:
        pn = np.ones_like(lg) if pen is None else np.asarray(pen, np.float32).reshape(-1)
        tok = int(np.argmax((lg * pn).astype(np.float32)))
        only = np.zeros(codes, bool)
        only[tok] = True
        return dict(token=tok, u=u, K=only, P=only.copy(), probs=only.astype(np.float64), margin=np.inf)
    z = z32(lg, None if pen is None else np.asarray(pen, np.float32).reshape(-1), temperature)
    if 0 < top_k < codes:
        t_k = np.sort(z)[::-1][top_k - 1]
        K = z >= t_k
    else:
        K = np.ones(codes, bool)
    z64 = z.astype(np.float64)
    e = np.where(K, np.exp(z64 - z64.max()), 0.0)
    S = e.sum()
    margin_p = np.inf
    tp = float(np.float32(top_p))
    if tp >= 1.0:
        P = K.copy()
    else:
        kidx = np.flatnonzero(K)
        order = kidx[np.argsort(-z64[kidx], kind="stable")]            # K by descending z
        zs, cs = z[order], np.cumsum(e[order])
        ends = np.flatnonzero(np.append(zs[1:] != zs[:-1], True))     # last member of every group of equal z
        vals, cum = zs[ends], cs[ends]                                # distinct values, mass of {z >= v}
        target = tp * S
        i = int(np.argmax(cum >= target)) if (cum >= target).any() else len(vals) - 1
        P = K & (z >= vals[i])
        below = cum[i - 1] if i > 0 else 0.0
        margin_p = min(abs(cum[i] - target), abs(target - below)) / target
    eP = np.where(P, e, 0.0)
    cdf = np.cumsum(eP)
    S_P = cdf[-1]
    idx = np.flatnonzero(P)
    hit = idx[cdf[idx] > float(u) * S_P]
    tok = int(hit[0]) if hit.size else int(idx[-1])
    edges = np.concatenate([[0.0], cdf[idx] / S_P])
    margin_u = float(np.abs(edges - float(u)).min())
    return dict(token=tok, u=u, K=K, P=P, probs=eP / S_P, margin=min(margin_p, margin_u))


def bookkeeping(tokens, codes, repeat_value, penalty_range, stop_tokens, pen=None):
    """The reference loop's penalty bookkeeping (Inference_IndexTTS_ONNX.py:756-772) applied to a given token stream: returns
    the penalty vector in front of every step (list of float32 (codes,)) and the one left at the end."""
    pen = np.ones(codes, np.float32) if pen is None else np.asarray(pen, np.float32).reshape(-1).copy()
    before, reset = [], 0
    toks = [int(t) for t in tokens]
    for n, t in enumerate(toks):
        before.append(pen.copy())
        if t in stop_tokens:
            break
        pen[t] = np.float32(repeat_value)
        if n + 1 > penalty_range and toks[reset] != t:
            pen[toks[reset]] = 1.0
            reset += 1
    return before, pen


def find_seed(logits, pen, temperature, top_k, top_p, n, start, eps=1e-4, tries=64):
    """The first seed >= start for which the case is not borderline at eps (z and u are exactly reproducible, so this is
    decided here, without the device).  Returns (seed, the reference result), or None if `tries` seeds were all borderline
    (the top-p margin does not depend on the seed)."""
    for seed in range(int(start), int(start) + tries):
        r = sample(logits, pen, temperature, top_k, top_p, seed, n)
        if r["margin"] >= eps:
            return seed, r
    return None


# ---- the shared cases of tests/test_gpt_sampling_ref.py (CPU) and tests/test_gpu_gpt_sampling.py ---------------------------
CASE_SEED = 20240917
CODES = (37, 301, 1025, 8194)
TOP_P = (0.05, 0.5, 0.8, 1.0)
TEMPS = (0.7, 1.0, 1.5)
ROWS = 16


def top_ks(codes):
    return (0, 1, 2, 30, codes - 1, codes)


def combos(codes):
    return [(k, p, t) for k in top_ks(codes) for p in TOP_P for t in TEMPS]


def _candidate_row(codes, r, cand):
    """A bulk of N(-2, 1.5^2) logits under a few peaks of U(8, 16) (an acoustic GPT's step: a handful of plausible codes), a tenth
    of the codes with a penalty of 0.7, negative logits among them (the reference's multiply makes those MORE likely).  The
    peaks carry ~99 % of the mass at every temperature used, so that u rarely falls among the densely packed CDF edges of the
    bulk, where every case would be borderline."""
    rng = np.random.default_rng([CASE_SEED, codes, r, cand])
    logits = (rng.standard_normal(codes) * 1.5 - 2.0).astype(np.float32)
    npk = max(4, min(40, codes // 8))
    at = rng.choice(codes, npk, replace=False)
    logits[at] = rng.uniform(8.0, 16.0, npk).astype(np.float32)
    pen = np.where(rng.random(codes) < 0.1, np.float32(0.7), np.float32(1.0)).astype(np.float32)
    return logits, pen


_cache = {}


def cases(codes):
    """The unit cases of one code count, computed once: dict(logits (16, codes), pen (16, codes), refs = {(top_k, top_p,
    temperature): (seeds uint64 (16,), positions int64 (16,), [reference result per row])}).  Rows and seeds are the first
    candidates, in a fixed order from CASE_SEED, for which the REFERENCE is not borderline at eps = 1e-4 in any combination."""
    if codes in _cache:
        return _cache[codes]
    L, Pn, refs = [], [], {c: ([], [], []) for c in combos(codes)}
    for r in range(ROWS):
        for cand in range(1000):
            logits, pen = _candidate_row(codes, r, cand)
            found = {}
            for (k, p, t) in combos(codes):
                n = (r * 37 + k) % 800
                got = find_seed(logits, pen, t, k, p, n, CASE_SEED * 1000 + r * 4096)
                if got is None:
                    break
                found[(k, p, t)] = (got[0], n, got[1])
            else:
                break
        else:
            raise AssertionError("no candidate row without a borderline combination")
        L.append(logits); Pn.append(pen)
        for c, (sd, n, ref) in found.items():
            refs[c][0].append(sd); refs[c][1].append(n); refs[c][2].append(ref)
    out = dict(logits=np.stack(L), pen=np.stack(Pn),
               refs={c: (np.asarray(v[0], np.uint64), np.asarray(v[1], np.int64), v[2]) for c, v in refs.items()})
    _cache[codes] = out
    return out


def tie_row(codes=1025):
    """logits quantised to steps of 0.25: many exact ties straddle t_k and t_p"""
    rng = np.random.default_rng(CASE_SEED + 1)
    return (np.round(rng.standard_normal(codes) * 1.5 * 4.0) / 4.0).astype(np.float32)


def freq_row(codes=301):
    rng = np.random.default_rng(CASE_SEED + 2)
    return (rng.standard_normal(codes) * 2.0).astype(np.float32)


FREQ_SEED, FREQ_N = 77, 4096


def freq_ok(tokens, ref):
    """every code of P within 5 binomial standard deviations of its probability over len(tokens) draws, nothing outside P"""
    n = len(tokens)
    counts = np.bincount(np.asarray(tokens), minlength=ref["P"].size)
    if counts[~ref["P"]].any():
        return False
    p = ref["probs"][ref["P"]]
    return bool((np.abs(counts[ref["P"]] - n * p) <= 5.0 * np.sqrt(n * p * (1.0 - p))).all())
