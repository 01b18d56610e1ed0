"""IndexTTS acoustic GPT-2: host-side mirror of the reference's graphs B, C, D, E and of the per-sentence decode loop.

``IndexGPT`` is what ``ort_session_B/_C/_D/_E`` are in /root/reference IndexTTS/Inference_IndexTTS_ONNX.py:619-675
(graph definitions: IndexTTS/Export_IndexTTS.py:203-289), executed by hand-written gfx950 kernels through the C-ABI:

    text_embed(text_ids)                      graph B   (:723-727)
    mel_embed(gpt_id, gen_len)                graph C   (:729-734, :775-780)
    concat(conds_latent, text_h, mel_h)       graph D   (:736-742)  — a host concatenate, nothing to accelerate
    step(hidden_state, ...)                   graph E   (:754)      — KV cache resident in the handle
    generate(conds_latent, text_ids)          the loop  (:716-783)  — all tokens without leaving the device

There is no CPU fallback: without libmi355tts.so and an MI355X every call raises.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _lib
from .config import IndexGPTConfig
from .weights import pack_gpt


@dataclass(frozen=True)
class Sampling:
    """How ``IndexGPT.generate*`` chooses each mel code (include/mi355tts.h, "sampling"): temperature, top-k (0 = every
    code, 1 = greedy), top-p and a 64-bit seed.  The defaults are upstream IndexTTS's.  The draw for a sentence's n-th token
    depends on (seed, n) alone: one seed gives one take, whatever batch the sentence is decoded in."""
    temperature: float = 1.0
    top_k: int = 30
    top_p: float = 0.8
    seed: int = 0

    def __post_init__(self):
        t, p = float(self.temperature), float(self.top_p)
        if not (math.isfinite(t) and t > 0.0):
            raise ValueError(f"temperature must be finite and > 0, got {self.temperature}")
        if int(self.top_k) != self.top_k or self.top_k < 0:
            raise ValueError(f"top_k must be an integer >= 0 (0 = every code), got {self.top_k}")
        if not (math.isfinite(p) and 0.0 < p <= 1.0):
            raise ValueError(f"top_p must be in (0, 1], got {self.top_p}")
        if int(self.seed) != self.seed or not 0 <= self.seed < 2 ** 64:
            raise ValueError(f"seed must be an integer in [0, 2^64), got {self.seed}")


_GREEDY = Sampling(1.0, 1, 1.0, 0)


def _sampling_arrays(items):
    """list of Sampling (None = greedy) -> the four host arrays of the batched C-ABI entries"""
    it = [_GREEDY if x is None else x for x in items]
    return (np.ascontiguousarray([x.temperature for x in it], dtype=np.float32),
            np.ascontiguousarray([x.top_k for x in it], dtype=np.int32),
            np.ascontiguousarray([x.top_p for x in it], dtype=np.float32),
            np.ascontiguousarray([x.seed for x in it], dtype=np.uint64))


def _batch_sampling(sampling, nb):
    """generate_batch*'s ``sampling`` argument -> None (all greedy) or a list of nb Sampling / None"""
    if sampling is None:
        return None
    items = [sampling] * nb if isinstance(sampling, Sampling) else list(sampling)
    if len(items) != nb or not all(x is None or isinstance(x, Sampling) for x in items):
        raise ValueError(f"sampling must be one Sampling or a list of {nb} Sampling / None")
    return None if all(x is None for x in items) else items


def sample_logits(logits, *, temperature, top_k, top_p, seeds, positions, pen=None, return_probs: bool = False):
    """The decode step's sampler on rows of logits (unit entry mi_gpt_sample_logits).  logits (rows, codes); the parameters
    are scalars or sequences of ``rows`` entries; positions = each row's decode index n.  Returns (tokens int32 (rows,),
    u float32 (rows,)[, probabilities float32 (rows, codes): e / S_P on the kept set, 0 elsewhere])."""
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    if lg.ndim != 2:
        raise ValueError("logits must be (rows, codes)")
    rows, codes = lg.shape
    pn = None
    if pen is not None:
        pn = np.ascontiguousarray(np.broadcast_to(np.asarray(pen, np.float32), lg.shape))
    T = np.ascontiguousarray(np.broadcast_to(np.asarray(temperature, np.float32), (rows,)))
    K = np.ascontiguousarray(np.broadcast_to(np.asarray(top_k, np.int32), (rows,)))
    Pp = np.ascontiguousarray(np.broadcast_to(np.asarray(top_p, np.float32), (rows,)))
    Sd = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, np.uint64), (rows,)))
    Ps = np.ascontiguousarray(np.broadcast_to(np.asarray(positions, np.int64), (rows,)))
    toks = np.zeros((rows,), np.int32)
    u = np.zeros((rows,), np.float32)
    probs = np.zeros((rows, codes), np.float32) if return_probs else None
    _lib.check(_lib.load().mi_gpt_sample_logits(
        lg.ctypes.data, None if pn is None else pn.ctypes.data, rows, codes, T.ctypes.data, K.ctypes.data, Pp.ctypes.data,
        Sd.ctypes.data, Ps.ctypes.data, toks.ctypes.data, u.ctypes.data, None if probs is None else probs.ctypes.data,
        _lib.MI_HOST), "mi_gpt_sample_logits")
    return (toks, u, probs) if return_probs else (toks, u)


def queue_schedule(prompt_rows, max_new, lengths, slots, max_seq, *, beams: int = 1):
    """Host model of ``mi_gpt_generate_queue``'s scheduling policy (include/mi355tts.h, "sentence queue") -> (steps, passes).

    prompt_rows / max_new: per sentence, as given to the entry; lengths: what each sentence actually produced (<= max_new; 0
    where max_new is 0); slots = the handle's max_batch; max_seq = the packed-row capacity of a prompt pass.  ``steps`` is
    the number of batched decode steps the entry launches (its stats[0]); ``passes`` lists every prompt pass as a list of
    (sentence, slot) in packing order.  beams = B: the schedule of the queue with beam search, which is this one over groups —
    ``slots // B`` units, a pass entry naming (sentence, group), group g being slots gB .. gB + B - 1.  Pure host code: it documents the policy, feeds tools/gpt_queue_bench.py and is what the
    tests hold the entry's stats against."""
    beams = int(beams)
    if beams < 1:
        raise ValueError("queue_schedule: beams must be >= 1")
    slots = int(slots) // beams
    rows = [int(r) for r in prompt_rows]
    limit = [int(m) for m in max_new]
    length = [int(x) for x in lengths]
    n = len(rows)
    if not (len(limit) == n and len(length) == n and n >= 1 and slots >= 1):
        raise ValueError("queue_schedule: prompt_rows, max_new and lengths must have one entry per sentence, slots >= 1")
    for i in range(n):
        if rows[i] < 1 or limit[i] < 0 or not (0 <= length[i] <= limit[i]) or (limit[i] > 0 and length[i] < 1):
            raise ValueError(f"queue_schedule: sentence {i}: rows {rows[i]}, max_new {limit[i]}, length {length[i]}")
    S = min(int(slots), n)
    owner = [-1] * S                      # the sentence in each slot
    got = [0] * n                         # tokens so far
    nxt, steps, passes = 0, 0, []

    def skip_empty(i):
        while i < n and limit[i] == 0:
            i += 1
        return i

    nxt = skip_empty(nxt)
    while True:
        # 1. admit
        while -1 in owner and nxt < n:
            this, total = [], 0
            while -1 in owner and nxt < n:
                if this and total + rows[nxt] > max_seq:
                    break
                slot = owner.index(-1)
                owner[slot] = nxt
                got[nxt] = 1              # the pass gives token 0
                this.append((nxt, slot))
                total += rows[nxt]
                nxt = skip_empty(nxt + 1)
            passes.append(this)
        # 2. retire
        freed = False
        for b in range(S):
            i = owner[b]
            if i >= 0 and got[i] >= length[i]:
                owner[b] = -1
                freed = True
        if freed and nxt < n:
            continue
        # 3. finish or decode
        live = [i for i in owner if i >= 0]
        if not live:
            return steps, passes
        c = min(16, min(limit[i] - got[i] for i in live))
        steps += c
        for i in live:
            got[i] = min(length[i], got[i] + c)


def lockstep_steps(lengths, slots):
    """Batched decode steps of the yardstick ``queue_schedule`` is compared with: ``generate_batch`` over index-order groups of
    ``slots`` sentences, each group decoding in 16-step chunks until its longest member is done."""
    ls = [int(x) for x in lengths]
    steps = 0
    for g in range(0, len(ls), int(slots)):
        longest = max(ls[g:g + int(slots)])
        if longest > 1:
            steps += 16 * -(-(longest - 1) // 16)
    return steps


MAX_BEAMS = 8


def _check_beams(beams, nb, cfg, sampling=None, pool=False):
    """The ``beams`` keyword of ``IndexGPT.generate*`` (include/mi355tts.h, "beam search"): an integer in [1, 8], not above the
    code count, nb * beams slots within the engine's max_batch, and together with ``sampling`` only in pool mode."""
    if isinstance(beams, bool) or int(beams) != beams or not 1 <= beams <= MAX_BEAMS:
        raise ValueError(f"beams must be an integer in [1, {MAX_BEAMS}], got {beams}")
    beams = int(beams)
    if beams > 1:
        if sampling is not None and not pool:
            raise ValueError("beams and sampling do not combine without pool=True: that beam search is deterministic")
        if beams > cfg.mel_codes:
            raise ValueError(f"beams = {beams} exceeds the {cfg.mel_codes} mel codes")
        if nb * beams > cfg.max_batch:
            raise ValueError(f"{nb} sentence(s) x {beams} beams need {nb * beams} slots; this engine was created with "
                             f"max_batch = {cfg.max_batch}")
    return beams


def beam_select(logits, prev_scores=None, *, beams: int, first: bool = False, pen=None):
    """One beam selection on rows of logits (unit entry mi_gpt_beam_select).  logits (groups * beams, codes), pen likewise or
    None (= ones), prev_scores (groups * beams,) — ignored when ``first`` (selection 0: only each group's first row is read).
    Returns (parents, tokens, scores), each (groups, beams): the new hypotheses best first, parents as rows inside the group."""
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    if lg.ndim != 2 or beams < 1 or lg.shape[0] % beams:
        raise ValueError("logits must be (groups * beams, codes)")
    rows, codes = lg.shape
    pn = None if pen is None else np.ascontiguousarray(np.broadcast_to(np.asarray(pen, np.float32), lg.shape))
    pv = None
    if not first:
        pv = np.ascontiguousarray(np.asarray(prev_scores, np.float32).reshape(-1))
        if pv.size != rows:
            raise ValueError(f"prev_scores must hold {rows} values")
    par = np.zeros((rows,), np.int32)
    tok = np.zeros((rows,), np.int32)
    sc = np.zeros((rows,), np.float32)
    _lib.check(_lib.load().mi_gpt_beam_select(
        lg.ctypes.data, None if pn is None else pn.ctypes.data, None if pv is None else pv.ctypes.data, rows // beams, int(beams),
        codes, int(bool(first)), par.ctypes.data, tok.ctypes.data, sc.ctypes.data, _lib.MI_HOST), "mi_gpt_beam_select")
    g = rows // beams
    return par.reshape(g, beams), tok.reshape(g, beams), sc.reshape(g, beams)


def beam_pool_select(logits, prev_scores, *, beams: int, n: int, max_new: int, stop_tokens=(), pool_scores, pool_finished,
                     open: bool = True, length_penalty: float = 0.0, early_stopping: bool = False, sampling=None, pen=None):
    """One pool-mode selection of one sentence (unit entry mi_gpt_beam_pool_select; include/mi355tts.h, "beam search with a
    finished pool").  logits (beams, codes), pen likewise or None, prev_scores (beams,) (ignored at n == 0), pool_scores /
    pool_finished (beams,), sampling a Sampling or None.  Returns a dict: cand / cand_acc / cand_stop (K,) in candidate order,
    parents / tokens / scores (beams,) of the next running hypotheses, pool_scores / pool_finished / pool_src (beams,) after
    the merge (pool_src: -1 - j = the entry that was at place j, q >= 0 = candidate q), open, done."""
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    if lg.ndim != 2 or lg.shape[0] != beams:
        raise ValueError("logits must be (beams, codes)")
    B, codes = lg.shape
    pn = None if pen is None else np.ascontiguousarray(np.broadcast_to(np.asarray(pen, np.float32), lg.shape))
    pv = None if prev_scores is None else np.ascontiguousarray(np.asarray(prev_scores, np.float32).reshape(-1))
    if pv is not None and pv.size != B:
        raise ValueError(f"prev_scores must hold {B} values")
    stops = np.ascontiguousarray(list(stop_tokens), dtype=np.int32)
    K = (stops.size + 1) * B
    ps = np.ascontiguousarray(np.asarray(pool_scores, np.float32).reshape(-1)).copy()
    pf = np.ascontiguousarray(np.asarray(pool_finished).reshape(-1).astype(np.int32))
    if ps.size != B or pf.size != B:
        raise ValueError(f"pool_scores and pool_finished must hold {B} values")
    op, dn = np.array([int(bool(open))], np.int32), np.zeros((1,), np.int32)
    sa = None if sampling is None else _sampling_arrays([sampling])
    cand, cacc, cstop = np.zeros((max(K, 1),), np.int32), np.zeros((max(K, 1),), np.float32), np.zeros((max(K, 1),), np.int32)
    par, tok, src = np.zeros((B,), np.int32), np.zeros((B,), np.int32), np.zeros((B,), np.int32)
    sc = np.zeros((B,), np.float32)
    _lib.check(_lib.load().mi_gpt_beam_pool_select(
        lg.ctypes.data, None if pn is None else pn.ctypes.data, None if pv is None else pv.ctypes.data, B, codes, int(n),
        int(max_new), stops.ctypes.data if stops.size else None, stops.size, ps.ctypes.data, pf.ctypes.data, op.ctypes.data,
        float(length_penalty), int(early_stopping), *((None,) * 4 if sa is None else (a.ctypes.data for a in sa)),
        cand.ctypes.data, cacc.ctypes.data, cstop.ctypes.data, par.ctypes.data, tok.ctypes.data, sc.ctypes.data, src.ctypes.data,
        dn.ctypes.data, _lib.MI_HOST), "mi_gpt_beam_pool_select")
    return dict(cand=cand[:K], cand_acc=cacc[:K], cand_stop=cstop[:K].astype(bool), parents=par, tokens=tok, scores=sc,
                pool_scores=ps, pool_finished=pf.astype(bool), pool_src=src, open=bool(op[0]), done=bool(dn[0]))


def _attn_inputs(q, K, V, slots: bool):
    """q (rows, hidden) -> a qkv array whose k / v thirds are zero (the kernels read q alone); K / V caches as float32"""
    q = np.asarray(q, np.float32)
    K = np.ascontiguousarray(K, dtype=np.float32)
    V = np.ascontiguousarray(V, dtype=np.float32)
    if q.ndim != 2 or q.shape[1] % 64 or K.shape != V.shape or K.ndim != (4 if slots else 3) or K.shape[-1] != 64 \
            or K.shape[-3] * 64 != q.shape[1]:
        raise ValueError("q must be (rows, 64 * heads), K / V " + ("(slots, heads, max_seq, 64)" if slots else "(heads, max_seq, 64)"))
    qkv = np.zeros((q.shape[0], 3 * q.shape[1]), np.float32)
    qkv[:, :q.shape[1]] = q
    return qkv, K, V, np.zeros(q.shape, np.float32)


def attention_decode(q, K, V, hist, *, dtype: str = "f32"):
    """The decode step's attention launch (unit entry mi_gpt_attn_decode): row r of q (slots, hidden) against keys
    0 .. min(hist[r] + 1, max_seq) - 1 of slot r of the caches K / V (slots, heads, max_seq, 64) -> (slots, hidden) float32."""
    qkv, K, V, out = _attn_inputs(q, K, V, True)
    h = np.ascontiguousarray(hist, dtype=np.int32).reshape(-1)
    if h.size != K.shape[0] or qkv.shape[0] != K.shape[0]:
        raise ValueError("one q row and one hist entry per slot")
    _lib.check(_lib.load().mi_gpt_attn_decode(qkv.ctypes.data, K.ctypes.data, V.ctypes.data, _lib.DTYPES[dtype], K.shape[1],
                                              K.shape[2], K.shape[0], h.ctypes.data, out.ctypes.data, _lib.MI_HOST),
               "mi_gpt_attn_decode")
    return out


def attention_decode_beam(q, K, V, hist, ndec, anc, *, beams: int, dtype: str = "f32"):
    """The beam step's attention launch (unit entry mi_gpt_attn_decode_beam): as attention_decode, with key j of slot r read
    from the group's first slot below P = hist[r] - ndec[r] + 1 and from slot anc[ndec[r] & 1, r, j - P] of the group from
    there on; anc (2, slots, max_seq) int32 with entries in [0, beams)."""
    qkv, K, V, out = _attn_inputs(q, K, V, True)
    ns, S = K.shape[0], K.shape[2]
    h = np.ascontiguousarray(hist, dtype=np.int32).reshape(-1)
    n = np.ascontiguousarray(ndec, dtype=np.int32).reshape(-1)
    a = np.ascontiguousarray(anc, dtype=np.int32)
    if h.size != ns or n.size != ns or qkv.shape[0] != ns or a.shape != (2, ns, S):
        raise ValueError("one q row, hist and ndec entry per slot; anc must be (2, slots, max_seq)")
    _lib.check(_lib.load().mi_gpt_attn_decode_beam(qkv.ctypes.data, K.ctypes.data, V.ctypes.data, _lib.DTYPES[dtype], K.shape[1], S,
                                                   ns, h.ctypes.data, n.ctypes.data, int(beams), a.ctypes.data, out.ctypes.data,
                                                   _lib.MI_HOST), "mi_gpt_attn_decode_beam")
    return out


def attention_prompt(q, K, V, hist: int, *, flag: int = 1, dtype: str = "f32"):
    """A lone prompt pass's attention launch (unit entry mi_gpt_attn_prompt): the rows of q (rows, hidden) are the new block
    behind ``hist`` cached rows of ONE slot's K / V (heads, max_seq, 64); additive mask -128 * flag on keys j > i."""
    qkv, K, V, out = _attn_inputs(q, K, V, False)
    _lib.check(_lib.load().mi_gpt_attn_prompt(qkv.ctypes.data, K.ctypes.data, V.ctypes.data, _lib.DTYPES[dtype], K.shape[0],
                                              K.shape[1], int(hist), qkv.shape[0], int(flag), out.ctypes.data, _lib.MI_HOST),
               "mi_gpt_attn_prompt")
    return out


def attention_prompt_packed(q, K, V, segs, *, dtype: str = "f32"):
    """The packed prompt pass's attention launch (unit entry mi_gpt_attn_prompt_packed): q (total, hidden) holds the segments
    ``segs`` = [(first, rows, slot)] back to back, each a prompt of its own in its slot of K / V (slots, heads, max_seq, 64)."""
    qkv, K, V, out = _attn_inputs(q, K, V, True)
    sg = np.ascontiguousarray(segs, dtype=np.int32).reshape(-1, 3)
    _lib.check(_lib.load().mi_gpt_attn_prompt_packed(qkv.ctypes.data, K.ctypes.data, V.ctypes.data, _lib.DTYPES[dtype], K.shape[1],
                                                     K.shape[2], K.shape[0], sg.ctypes.data, sg.shape[0], qkv.shape[0],
                                                     out.ctypes.data, _lib.MI_HOST), "mi_gpt_attn_prompt_packed")
    return out


def _f32(a, shape=None, what=""):
    """None stays None; otherwise a contiguous float32 array (of ``shape`` when given)"""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError(f"{what} must have shape {tuple(shape)}, not {a.shape}")
    return a


def _ptr(a):
    return None if a is None else a.ctypes.data


def _q8_arrays(q8, what):
    """(q (n, k) uint8, scale (n) float32, zp (n) uint8), contiguous"""
    q, scale, zp = q8
    q = np.ascontiguousarray(q, dtype=np.uint8)
    if q.ndim != 2:
        raise ValueError(f"{what}: q must be (n, k)")
    scale = np.ascontiguousarray(scale, dtype=np.float32)
    zp = np.ascontiguousarray(zp, dtype=np.uint8)
    if scale.shape != (q.shape[0],) or zp.shape != (q.shape[0],):
        raise ValueError(f"{what}: scale and zp must have one entry per row of q")
    return q, scale, zp


def linear_decode(w, x, *, bias=None, ln=None, pre=None, res=None, act: bool = False, out_f32: bool = True, cache=None,
                  hist: int = 0, dtype: str = "f32", q8=None):
    """One decode-step linear launch of ONE sentence (unit entry mi_gpt_linear_decode, csrc/gpt.hip gemv_d_kernel):
    act(w x' + bias) + res for w (n, k), x (k).  ``ln`` = (gain, shift): x stays float32 and x' = LayerNorm(x); ``pre`` = (gain,
    shift) of a LayerNorm in front of that one, whose row is returned too.  ``cache`` = (K, V), one layer's caches
    (k / 64, max_seq, 64): the QKV form (n = 3 k) — columns [k, 3k) go to row ``hist`` of copies of K and V, not to the output.
    ``q8`` = (q, scale, zp) with ``w`` None: per-channel uint8 weights (mi_gpt_linear_decode_q8, csrc/gpt_q8.hip), dtype "f16".
    Returns a dict: "out" (n) float32, NaN where the launch wrote nothing; "pre_out" (k) with ``pre``; "K", "V" with ``cache``."""
    if q8 is not None:
        if w is not None:
            raise ValueError("give w or q8, not both")
        q8 = _q8_arrays(q8, "linear_decode")
        n, k = q8[0].shape
    else:
        w = _f32(w)
        if w.ndim != 2:
            raise ValueError("w must be (n, k)")
        n, k = w.shape
    x = _f32(x, (k,), "x")
    bias, res = _f32(bias, (n,), "bias"), _f32(res, (n,), "res")
    lw, lb = (_f32(ln[0], (k,), "ln gain"), _f32(ln[1], (k,), "ln shift")) if ln is not None else (None, None)
    pw, pb = (_f32(pre[0], (k,), "pre gain"), _f32(pre[1], (k,), "pre shift")) if pre is not None else (None, None)
    out = np.zeros(n, np.float32)
    pre_out = np.zeros(k, np.float32) if pre is not None else None
    K = V = None
    S = 1
    if cache is not None:
        K, V = (np.array(c, dtype=np.float32, order="C") for c in cache)
        if K.shape != V.shape or K.ndim != 3 or K.shape[2] != 64:
            raise ValueError("cache = (K, V), each (heads, max_seq, 64)")
        S = K.shape[1]
    rest = (_ptr(bias), _ptr(x), _lib.DTYPES[dtype], n, k, _ptr(lw), _ptr(lb), _ptr(pw), _ptr(pb), _ptr(pre_out), _ptr(res),
            int(bool(act)), int(bool(out_f32)), int(cache is not None), int(hist), S, _ptr(K), _ptr(V), _ptr(out), _lib.MI_HOST)
    if q8 is not None:
        _lib.check(_lib.load().mi_gpt_linear_decode_q8(*(_ptr(a) for a in q8), *rest), "mi_gpt_linear_decode_q8")
    else:
        _lib.check(_lib.load().mi_gpt_linear_decode(_ptr(w), *rest), "mi_gpt_linear_decode")
    r = {"out": out}
    if pre is not None:
        r["pre_out"] = pre_out
    if cache is not None:
        r["K"], r["V"] = K, V
    return r


def linear_batch_rows(nb: int) -> int:
    """Rows of the batched decode scratch an engine of ``nb`` slots allocates (2, 4, 8, then multiples of 16)"""
    p = _lib.load().mi_gpt_linear_batch_rows(int(nb))
    if p < 0:
        raise ValueError("nb must be in [1, 64]")
    return p


def linear_batch(w, x, *, bias=None, res=None, act: bool = False, out_f32: bool = True, cache=None, hist=None, x_dead=None,
                 dtype: str = "f32", q8=None):
    """One batched decode-step linear launch (unit entry mi_gpt_linear_batch, csrc/gpt.hip gemv_b_kernel / gemm_skinny_kernel /
    gemm_skinny_wide_kernel by the engine's dispatch): row b of x (nb, k) is slot b.  ``cache`` = (K, V), (nb, k / 64, max_seq, 64)
    with ``hist`` (nb): the QKV form.  ``x_dead`` (k): what the device x array holds in its rows nb .. linear_batch_rows(nb) - 1.
    ``q8`` = (q, scale, zp) with ``w`` None: per-channel uint8 weights (mi_gpt_linear_batch_q8), dtype "f16".
    Returns a dict: "out" (linear_batch_rows(nb), n) float32 — rows >= nb are never written and come back NaN; "K", "V"."""
    if q8 is not None:
        if w is not None:
            raise ValueError("give w or q8, not both")
        q8 = _q8_arrays(q8, "linear_batch")
    else:
        w = _f32(w)
    x = _f32(x)
    wshape = q8[0].shape if q8 is not None else w.shape
    if len(wshape) != 2 or x.ndim != 2 or x.shape[1] != wshape[1]:
        raise ValueError("w must be (n, k), x (nb, k)")
    (n, k), nb = wshape, x.shape[0]
    bias, res, x_dead = _f32(bias, (n,), "bias"), _f32(res, (nb, n), "res"), _f32(x_dead, (k,), "x_dead")
    K = V = h = None
    S = 1
    if cache is not None:
        K, V = (np.array(c, dtype=np.float32, order="C") for c in cache)
        h = np.ascontiguousarray(hist, dtype=np.int32).reshape(-1)
        if K.shape != V.shape or K.ndim != 4 or K.shape[0] != nb or K.shape[3] != 64 or h.size != nb:
            raise ValueError("cache = (K, V), each (nb, heads, max_seq, 64), with one hist entry per row")
        S = K.shape[2]
    out = np.zeros((linear_batch_rows(nb), n), np.float32)
    rest = (_ptr(bias), _ptr(x), _ptr(x_dead), _lib.DTYPES[dtype], n, k, nb, _ptr(res), int(bool(act)), int(bool(out_f32)),
            int(cache is not None), _ptr(h), S, _ptr(K), _ptr(V), _ptr(out), _lib.MI_HOST)
    if q8 is not None:
        _lib.check(_lib.load().mi_gpt_linear_batch_q8(*(_ptr(a) for a in q8), *rest), "mi_gpt_linear_batch_q8")
    else:
        _lib.check(_lib.load().mi_gpt_linear_batch(_ptr(w), *rest), "mi_gpt_linear_batch")
    r = {"out": out}
    if cache is not None:
        r["K"], r["V"] = K, V
    return r


def _check_queue_beams(beams, cfg, sampling, pool=False, length_penalty=0.0, early_stopping=False):
    """The ``beams`` keyword of the queue entries: None (no beam search) or an integer in [1, 8], not above the code count or the
    engine's max_batch (one group must fit), and together with ``sampling`` only in pool mode.  ``pool`` needs ``beams``, and
    ``length_penalty`` / ``early_stopping`` belong to ``pool``."""
    if not pool and (length_penalty != 0.0 or early_stopping):
        raise ValueError("length_penalty and early_stopping belong to pool=True")
    if beams is None:
        if pool:
            raise ValueError("pool=True is a beam mode: give beams")
        return None
    if isinstance(beams, bool) or int(beams) != beams or not 1 <= beams <= MAX_BEAMS:
        raise ValueError(f"beams must be an integer in [1, {MAX_BEAMS}], got {beams}")
    if sampling is not None and not pool:
        raise ValueError("beams and sampling do not combine without pool=True: that beam search is deterministic")
    if pool and isinstance(sampling, (list, tuple)) and any(x is None for x in sampling) and any(x is not None for x in sampling):
        raise ValueError("pool mode samples every sentence of the call or none")
    if beams > cfg.mel_codes:
        raise ValueError(f"beams = {beams} exceeds the {cfg.mel_codes} mel codes")
    if beams > cfg.max_batch:
        raise ValueError(f"{beams} beams need {beams} slots; this engine was created with max_batch = {cfg.max_batch}")
    return int(beams)


def _queue_beam_call(handle, cfg, cat, rows, mx, stops, repeat_value, penalty_range, cap, beams, pool=None):
    """mi_gpt_generate_queue_beam on host arrays -> (tokens, hidden, counts, scores, stats); with pool = (length_penalty,
    early_stopping, sampling arrays or None) mi_gpt_generate_queue_beam_pool.  What the entry rejects before launching anything
    (MI_EINVAL) is a ValueError; the handle stays usable."""
    n = int(rows.size)
    toks = np.zeros((n, cap), np.int32)
    hid = np.zeros((n, cap, cfg.hidden), np.float32)
    cnt = np.zeros((n,), np.int32)
    sc = np.zeros((n,), np.float32)
    stats = np.zeros((2,), np.int32)
    L = _lib.load()
    head = (handle, n, cat.ctypes.data, _lib.i32p(rows), _lib.i32p(mx), stops.ctypes.data if stops.size else None, stops.size,
            repeat_value, penalty_range, int(beams))
    tail = (toks.ctypes.data, hid.ctypes.data, cap, _lib.i32p(cnt), sc.ctypes.data, _lib.MI_HOST, stats.ctypes.data)
    if pool is None:
        name = "mi_gpt_generate_queue_beam"
        rc = L.mi_gpt_generate_queue_beam(*head, *tail)
    else:
        name = "mi_gpt_generate_queue_beam_pool"
        lp, es, sa = pool
        rc = L.mi_gpt_generate_queue_beam_pool(*head, float(lp), int(bool(es)),
                                               *((None,) * 4 if sa is None else (a.ctypes.data for a in sa)), *tail)
    if rc == _lib.MI_EINVAL:
        raise ValueError(name + ": " + L.mi_last_error().decode("utf-8", "replace"))
    _lib.check(rc, name)
    return toks, hid, cnt, sc, stats


def _queue_call(handle, cfg, cat, rows, mx, stops, repeat_value, penalty_range, cap, sampling_arrays):
    """mi_gpt_generate_queue on host arrays.  sampling_arrays: None or (temperature, top_k, top_p, seeds), an item of which may
    be None.  What the entry rejects before launching anything (MI_EINVAL) is a ValueError; the handle stays usable."""
    n = int(rows.size)
    toks = np.zeros((n, cap), np.int32)
    hid = np.zeros((n, cap, cfg.hidden), np.float32)
    cnt = np.zeros((n,), np.int32)
    stats = np.zeros((2,), np.int32)
    sa = (None,) * 4 if sampling_arrays is None else tuple(sampling_arrays)
    L = _lib.load()
    rc = L.mi_gpt_generate_queue(handle, n, cat.ctypes.data, _lib.i32p(rows), _lib.i32p(mx),
                                 stops.ctypes.data if stops.size else None, stops.size, repeat_value, penalty_range,
                                 toks.ctypes.data, hid.ctypes.data, cap, _lib.i32p(cnt), _lib.MI_HOST,
                                 *(None if a is None else a.ctypes.data for a in sa), _lib.i32p(stats))
    if rc == _lib.MI_EINVAL:
        raise ValueError("mi_gpt_generate_queue: " + L.mi_last_error().decode("utf-8", "replace"))
    _lib.check(rc, "mi_gpt_generate_queue")
    return toks, hid, cnt, stats


class QueueSession:
    """An open sentence-queue session (include/mi355tts.h, mi_gpt_queue_begin / _advance / _end; made by
    ``IndexGPT.queue_session``).  ``tokens`` (n, cap) int32 and ``hidden`` (n, cap, hidden) float32 are numpy arrays, or torch
    tensors on the engine's device with device=True; after ``advance()`` the first count[i] entries of sentence i are valid and
    final.  With ``beams`` (mi_gpt_queue_begin_beam; with ``pool`` = (length_penalty, early_stopping) as well,
    mi_gpt_queue_begin_beam_pool, where the sampling arrays belong to the beam sampling) a sentence's count stays 0 until it is
    retired and is then all of it; ``scores`` (n,) float32 holds the score of every retired sentence's result (None without
    beams).  A context manager: leaving it ends the session (also before everything has finished)."""

    def __init__(self, gpt, cat, rows, mx, stops, repeat_value, penalty_range, cap, sampling_arrays, device, beams=None,
                 pool=None):
        self._gpt = gpt
        self._open = False
        c = gpt.cfg
        n = int(rows.size)
        self.n, self.cap = n, cap
        self._count = np.zeros((n,), np.int32)
        self._done = np.zeros((n,), np.int32)
        self._fin = np.zeros((1,), np.int32)
        self._stats = np.zeros((2,), np.int32)
        sa = (None,) * 4 if sampling_arrays is None else tuple(sampling_arrays)
        L = _lib.load()
        if device:
            import torch
            dev = torch.device("cuda", gpt.device)
            self._cat = torch.from_numpy(cat).to(dev)
            self._stops = torch.from_numpy(stops).to(dev) if stops.size else None
            self.tokens = torch.zeros((n, cap), dtype=torch.int32, device=dev)
            self.hidden = torch.zeros((n, cap, c.hidden), dtype=torch.float32, device=dev)
            self.scores = None if beams is None else torch.zeros((n,), dtype=torch.float32, device=dev)
            torch.cuda.current_stream(dev).synchronize()
            ptrs = (self._cat.data_ptr(), None if self._stops is None else self._stops.data_ptr(), self.tokens.data_ptr(),
                    self.hidden.data_ptr(), None if beams is None else self.scores.data_ptr())
            mem = _lib.MI_DEVICE
        else:
            self._cat, self._stops = cat, stops
            self.tokens = np.zeros((n, cap), np.int32)
            self.hidden = np.zeros((n, cap, c.hidden), np.float32)
            self.scores = None if beams is None else np.zeros((n,), np.float32)
            ptrs = (cat.ctypes.data, stops.ctypes.data if stops.size else None, self.tokens.ctypes.data, self.hidden.ctypes.data,
                    None if beams is None else self.scores.ctypes.data)
            mem = _lib.MI_HOST
        if beams is None:
            name = "mi_gpt_queue_begin"
            rc = L.mi_gpt_queue_begin(gpt._h, n, ptrs[0], _lib.i32p(rows), _lib.i32p(mx), ptrs[1], stops.size, repeat_value,
                                      penalty_range, ptrs[2], ptrs[3], cap, mem, *(None if a is None else a.ctypes.data for a in sa))
        elif pool is None:
            name = "mi_gpt_queue_begin_beam"
            rc = L.mi_gpt_queue_begin_beam(gpt._h, n, ptrs[0], _lib.i32p(rows), _lib.i32p(mx), ptrs[1], stops.size, repeat_value,
                                           penalty_range, int(beams), ptrs[2], ptrs[3], cap, ptrs[4], mem)
        else:
            name = "mi_gpt_queue_begin_beam_pool"
            rc = L.mi_gpt_queue_begin_beam_pool(gpt._h, n, ptrs[0], _lib.i32p(rows), _lib.i32p(mx), ptrs[1], stops.size,
                                                repeat_value, penalty_range, int(beams), float(pool[0]), int(bool(pool[1])),
                                                *(None if a is None else a.ctypes.data for a in sa), ptrs[2], ptrs[3], cap,
                                                ptrs[4], mem)
        if rc == _lib.MI_EINVAL:
            raise ValueError(name + ": " + L.mi_last_error().decode("utf-8", "replace"))
        _lib.check(rc, name)
        self._open = True

    def advance(self):
        """One round of the queue's policy: admissions and retirements, then one run of at most 16 decode steps.  Returns
        (count, done, finished): int32 (n,) valid tokens / rows per sentence, bool (n,) whether that is all of the sentence,
        and whether nothing is live or waiting any more.  With beams a sentence's count is 0 until the round that retires it."""
        if not self._open:
            raise _lib.MiError("the queue session has ended")
        _lib.check(_lib.load().mi_gpt_queue_advance(self._gpt._h, self._count.ctypes.data, self._done.ctypes.data,
                                                    self._fin.ctypes.data, self._stats.ctypes.data), "mi_gpt_queue_advance")
        return self._count.copy(), self._done.astype(bool), bool(self._fin[0])

    @property
    def stats(self):
        """{"steps": decode steps launched, "passes": prompt passes}, so far"""
        return {"steps": int(self._stats[0]), "passes": int(self._stats[1])}

    def end(self):
        if self._open:
            self._open = False
            if getattr(self._gpt, "_h", None):
                _lib.check(_lib.load().mi_gpt_queue_end(self._gpt._h), "mi_gpt_queue_end")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.end()
        return False

    def __del__(self):
        try:
            self.end()
        except Exception:
            pass


def stream_plan(emitted, count, done, chunk: int, halo: int):
    """Which vocoder windows are ready: the host model of ``stream_synthesize``.  emitted[i] = frames of sentence i already
    emitted, count[i] / done[i] = what ``QueueSession.advance`` reported.  A sentence has A = count - 2 frames available: its F
    when done, and safe while live (a live sentence's last two rows are not yet known to be frames).  While live a sentence emits
    [e, e + chunk) as soon as e + chunk + halo <= A, again and again; when done it emits everything left, [e, F), as one
    window.  Each piece [a, b) becomes the window of frames [lo, hi) = [max(0, a - halo), min(A, b + halo)) with head = a - lo
    and tail = hi - b.  Sentences with fewer than three codes emit nothing.  Returns (windows, emitted_after): windows = list of
    (sentence, a, b, lo, hi, last) in sentence order, pieces of a sentence in frame order."""
    chunk, halo = int(chunk), int(halo)
    if chunk < 1 or halo < 0:
        raise ValueError("stream_plan: chunk must be >= 1 and halo >= 0")
    if not (len(emitted) == len(count) == len(done)):
        raise ValueError("stream_plan: emitted, count and done must have one entry per sentence")
    out, after = [], [int(e) for e in emitted]
    for i in range(len(after)):
        A = int(count[i]) - 2
        e = after[i]
        if A < 1 or e >= A:
            continue
        if done[i]:
            pieces = [(e, A)]
        else:
            pieces = []
            while e + chunk + halo <= A:
                pieces.append((e, e + chunk))
                e += chunk
        for a, b in pieces:
            out.append((i, a, b, max(0, a - halo), min(A, b + halo), bool(done[i]) and b == A))
            after[i] = b
    return out, after


def stream_synthesize(gpt, voc, prompts, max_new, voices, voice_of, *, chunk: int = 32, halo: Optional[int] = None, **decode_kw):
    """Audio while the queue decodes: a generator over (sentence, first_sample, int16 chunk, last).  gpt = IndexGPT, voc = a
    graph-F BigVGANVocoder, prompts / max_new / decode_kw (stop_tokens, repeat_value, penalty_range, sampling, beams, pool,
    length_penalty, early_stopping) as
    ``IndexGPT.generate_queue``, voices / voice_of as ``BigVGANVocoder.run_latent_voices`` (one voice index per sentence).
    Every round is one ``QueueSession.advance()`` followed by ONE ``run_latent_windows_torch`` call over all windows
    ``stream_plan`` reports, of any sentences and voices, reading the rows from the session's device `hidden`.  The chunks of a
    sentence tile its waveform [0, F * hop + 30) in order, `last` on the final one; a sentence of fewer than three codes yields
    nothing.  With ``beams=B`` no row of a sentence is final before it ends, so every sentence leaves as ONE chunk (its whole
    waveform) in the round that retires it, while the other groups go on decoding.  halo: frames of context at each cut (default: ``voc.cfg.halo_frames()``, with which the samples are those of the
    whole sentence's forward; less trades accuracy for work).  One thread: the vocoder call pauses the decode."""
    import torch
    from .bigvgan import voices_table
    n = len(prompts)
    halo = voc.cfg.halo_frames() if halo is None else int(halo)
    table, index = voices_table(voc.cfg, voices, voice_of, n)
    hop = voc.cfg.hop
    with gpt.queue_session(prompts, max_new, device=True, **decode_kw) as q:
        tab = torch.from_numpy(table).to(q.hidden.device)
        emitted = [0] * n
        finished = False
        while not finished:
            count, done, finished = q.advance()
            plan, emitted = stream_plan(emitted, count, done, chunk, halo)
            if not plan:
                continue
            wins = [(i * q.cap + lo, hi - lo, a - lo, hi - b) for i, a, b, lo, hi, _ in plan]
            wav, lens = voc.run_latent_windows_torch(q.hidden, wins, tab, [int(index[i]) for i, *_ in plan])
            wav = wav.cpu().numpy()
            off = 0
            for (i, a, b, lo, hi, last), ln in zip(plan, lens):
                # the piece's own samples; the window's kept range is exactly that unless halo == 0 left a cut without a halo
                # frame (an untrimmed end carries the 15 + 15 samples of the post activation's padding)
                s0 = a * hop + 15 if a else 0
                s1 = b * hop + (30 if last else 15)
                k0 = lo * hop + ((a - lo) * hop + 15 if a > lo else 0)
                yield i, s0, wav[off + s0 - k0:off + s1 - k0].copy(), last
                off += ln


class IndexGPT:
    def __init__(self, cfg: IndexGPTConfig, state: Optional[dict] = None, *, blob: Optional[np.ndarray] = None,
                 blob_device=None, dtype: str = "f32", device: int = 0, weights: Optional[str] = None):
        """``weights="q8"``: the six matrix kinds held as per-channel uint8 and dequantised in the kernels (mi_gpt_create_q8;
        dtype "f16"), quantised at creation from the same fp32 state or blob; None: weights of ``dtype``."""
        if weights not in (None, "q8"):
            raise ValueError('weights must be None or "q8"')
        self.cfg = cfg
        self.dtype = dtype
        self.weights = weights
        self.device = device
        self._h = None
        L = _lib.load()
        _lib.init(device)
        self.repeat_penality = np.ones((1, cfg.mel_codes), np.float32)
        if blob_device is not None:          # packed fp32 blob as a CUDA tensor (e.g. filled by an RCCL broadcast)
            import torch
            t = blob_device
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device.index == device):
                raise ValueError("blob_device must be a contiguous float32 CUDA tensor on the engine's device")
            ci = np.asarray(cfg.to_int_array(), dtype=np.int32)
            torch.cuda.current_stream(t.device).synchronize()
            create = L.mi_gpt_create_q8 if weights == "q8" else L.mi_gpt_create_mem
            self._h = create(_lib.i32p(ci), len(ci), t.data_ptr(), t.numel(), _lib.DTYPES[dtype], device, _lib.MI_DEVICE)
            if not self._h:
                raise _lib.MiError(("mi_gpt_create_q8: " if weights == "q8" else "mi_gpt_create_mem: ") + L.mi_last_error().decode())
            return
        if blob is None:
            if state is None:
                raise ValueError("IndexGPT needs a state dict or a packed blob")
            blob = pack_gpt(cfg, state)
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        ci = np.asarray(cfg.to_int_array(), dtype=np.int32)
        expect = L.mi_gpt_param_count(_lib.i32p(ci), len(ci))
        if expect != blob.size:
            raise _lib.MiError(f"weight blob has {blob.size} floats, config needs {expect}")
        if weights == "q8":
            self._h = L.mi_gpt_create_q8(_lib.i32p(ci), len(ci), blob.ctypes.data, blob.size, _lib.DTYPES[dtype], device, _lib.MI_HOST)
            if not self._h:
                raise _lib.MiError("mi_gpt_create_q8: " + L.mi_last_error().decode())
        else:
            self._h = L.mi_gpt_create(_lib.i32p(ci), len(ci), _lib.f32p(blob), blob.size, _lib.DTYPES[dtype], device)
            if not self._h:
                raise _lib.MiError("mi_gpt_create: " + L.mi_last_error().decode())
        # the reference initialises repeat_penality once and carries it across sentences (:685)
        self.repeat_penality = np.ones((1, cfg.mel_codes), np.float32)

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().mi_gpt_destroy(self._h)
            self._h = None

    def weight_bytes(self) -> int:
        """device bytes held for the six matrix kinds (q8: bytes + scales + zero points + the prompt scratch)"""
        n = _lib.load().mi_gpt_weight_bytes(self._h)
        if n < 0:
            raise _lib.MiError("mi_gpt_weight_bytes: " + _lib.load().mi_last_error().decode())
        return int(n)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- graph B ------------------------------------------------------------------------------------------------
    def text_embed(self, text_ids) -> np.ndarray:
        ids = np.ascontiguousarray(np.asarray(text_ids).reshape(-1), dtype=np.int32)
        out = np.empty((1, ids.size + 2, self.cfg.hidden), np.float32)
        _lib.check(_lib.load().mi_gpt_text_embed(self._h, ids.ctypes.data, ids.size, out.ctypes.data, _lib.MI_HOST),
                   "mi_gpt_text_embed")
        return out

    # ---- graph C ------------------------------------------------------------------------------------------------
    def mel_embed(self, gpt_id, gen_len):
        g = int(np.asarray(gen_len).reshape(-1)[0])
        out = np.empty((1, 1, self.cfg.hidden), np.float32)
        _lib.check(_lib.load().mi_gpt_mel_embed(self._h, int(np.asarray(gpt_id).reshape(-1)[0]), g, out.ctypes.data,
                                                _lib.MI_HOST), "mi_gpt_mel_embed")
        return out, np.array([g + 1], np.int64)

    # ---- graph D ------------------------------------------------------------------------------------------------
    @staticmethod
    def concat(embed_x, embed_y, embed_z):
        c = np.ascontiguousarray(np.concatenate([embed_x, embed_y, embed_z], axis=1), dtype=np.float32)
        return c, np.array([c.shape[1]], np.int64)

    # ---- graph E ------------------------------------------------------------------------------------------------
    @property
    def history_len(self) -> int:
        return int(_lib.load().mi_gpt_history_len(self._h))

    def reset(self):
        _lib.check(_lib.load().mi_gpt_reset(self._h), "mi_gpt_reset")

    def step(self, hidden_state, repeat_penality=None, attention_mask: int = 0, return_logits: bool = False):
        """hidden_state (1, ids_len, hidden) appended after the handle's history.  Returns (kv_seq_len,
        last_hidden_state (1, hidden), max_logit_id (1, 1) int32[, logits (1, mel_codes)])."""
        hs = np.ascontiguousarray(hidden_state, dtype=np.float32)
        if hs.ndim != 3 or hs.shape[0] != 1 or hs.shape[2] != self.cfg.hidden or hs.shape[1] < 1:
            raise ValueError(f"hidden_state must be (1, ids_len >= 1, {self.cfg.hidden}), got {hs.shape}")
        pen = None
        if repeat_penality is not None:
            pen = np.ascontiguousarray(repeat_penality, dtype=np.float32).reshape(-1)
            if pen.size != self.cfg.mel_codes:
                raise ValueError(f"repeat_penality must hold {self.cfg.mel_codes} values")
        last = np.empty((1, self.cfg.hidden), np.float32)
        tok = np.empty((1, 1), np.int32)
        logits = np.empty((1, self.cfg.mel_codes), np.float32) if return_logits else None
        _lib.check(_lib.load().mi_gpt_step(self._h, hs.ctypes.data, hs.shape[1], None if pen is None else pen.ctypes.data,
                                           int(attention_mask), last.ctypes.data, tok.ctypes.data,
                                           None if logits is None else logits.ctypes.data, _lib.MI_HOST), "mi_gpt_step")
        kv = np.array([self.history_len], np.int64)
        return (kv, last, tok, logits) if return_logits else (kv, last, tok)

    def kv_read(self, layer: int):
        """(keys (H, 64, history), values (H, history, 64)) of one layer, in the reference's out_key_i / out_value_i
        layouts."""
        c, hist = self.cfg, self.history_len
        k = np.zeros((c.heads, c.head_dim, hist), np.float32)
        v = np.zeros((c.heads, hist, c.head_dim), np.float32)
        if hist:
            _lib.check(_lib.load().mi_gpt_kv_read(self._h, layer, k.ctypes.data, v.ctypes.data, _lib.MI_HOST),
                       "mi_gpt_kv_read")
        return k, v

    def kv_write(self, keys: Sequence[np.ndarray], values: Sequence[np.ndarray]):
        """Load a cache given as the reference's in_key_i / in_value_i lists; history_len := keys[0].shape[2]."""
        c = self.cfg
        if len(keys) != c.layers or len(values) != c.layers:
            raise ValueError(f"expected {c.layers} key and value tensors")
        hist = int(np.asarray(keys[0]).shape[2])
        for i in range(c.layers):
            k = np.ascontiguousarray(keys[i], dtype=np.float32)
            v = np.ascontiguousarray(values[i], dtype=np.float32)
            if k.shape != (c.heads, c.head_dim, hist) or v.shape != (c.heads, hist, c.head_dim):
                raise ValueError(f"layer {i}: keys {k.shape} / values {v.shape} do not match history {hist}")
            _lib.check(_lib.load().mi_gpt_kv_write(self._h, i, k.ctypes.data, v.ctypes.data, hist, _lib.MI_HOST),
                       "mi_gpt_kv_write")

    # ---- the per-sentence loop ------------------------------------------------------------------------------------
    def generate_from_prompt(self, prompt, max_new: int, *, stop_tokens=None, repeat_value=None, penalty_range=None,
                             repeat_penality=None, sampling: Optional[Sampling] = None, beams: int = 1):
        """prompt (1, P, hidden) = graph D's output.  Returns (tokens (n,), hidden (n, hidden), repeat_penality).
        sampling: a ``Sampling`` draws each token on the device; None decodes greedily like the reference.
        beams > 1: beam search with that many hypotheses (needs max_batch >= beams); the best hypothesis is returned."""
        c = self.cfg
        if _check_beams(beams, 1, c, sampling) > 1:
            res, pen = self.generate_beam([prompt], [max_new], beams, stop_tokens=stop_tokens, repeat_value=repeat_value,
                                          penalty_range=penalty_range,
                                          repeat_penality=self.repeat_penality if repeat_penality is None else repeat_penality)
            if repeat_penality is None:
                self.repeat_penality = pen
            return res[0][0], res[0][1], pen
        p = np.ascontiguousarray(prompt, dtype=np.float32)
        if p.ndim != 3 or p.shape[0] != 1 or p.shape[2] != c.hidden or p.shape[1] < 1:
            raise ValueError(f"prompt must be (1, P >= 1, {c.hidden}), got {p.shape}")
        stops = np.ascontiguousarray([c.stop_mel_token] if stop_tokens is None else list(stop_tokens), dtype=np.int32)
        pen = np.ascontiguousarray(self.repeat_penality if repeat_penality is None else repeat_penality,
                                   dtype=np.float32).reshape(1, -1).copy()
        max_new = int(max_new)
        toks = np.zeros((max(max_new, 1),), np.int32)
        hid = np.zeros((max(max_new, 1), c.hidden), np.float32)
        import ctypes as C
        n = C.c_int32(0)
        args = (self._h, p.ctypes.data, p.shape[1], max_new, stops.ctypes.data if stops.size else None, stops.size,
                float(c.repeat_penalty if repeat_value is None else repeat_value),
                int(c.penalty_range if penalty_range is None else penalty_range), pen.ctypes.data, toks.ctypes.data,
                hid.ctypes.data, C.byref(n), _lib.MI_HOST)
        if sampling is None:
            _lib.check(_lib.load().mi_gpt_generate(*args), "mi_gpt_generate")
        else:
            _lib.check(_lib.load().mi_gpt_generate_sampled(*args, float(sampling.temperature), int(sampling.top_k),
                                                           float(sampling.top_p), int(sampling.seed)),
                       "mi_gpt_generate_sampled")
        if repeat_penality is None:
            self.repeat_penality = pen
        return toks[: n.value].copy(), hid[: n.value].copy(), pen

    def generate_torch(self, prompt, max_new: int, tokens, hidden, *, stop_tokens=None, repeat_value=None,
                       penalty_range=None, repeat_penality=None, sampling: Optional[Sampling] = None, beams: int = 1) -> int:
        """Device-resident variant: prompt (P, hidden) float32 CUDA tensor; tokens (>= max_new) int32 and hidden
        (>= max_new, hidden) float32 CUDA tensors are filled; repeat_penality (mel_codes) float32 CUDA tensor or None
        (= ones, not written back).  Returns the number of tokens produced."""
        import ctypes as C
        import torch
        c = self.cfg
        beams = _check_beams(beams, 1, c, sampling)
        assert prompt.is_cuda and prompt.dtype == torch.float32 and prompt.is_contiguous() and prompt.shape[-1] == c.hidden
        assert tokens.is_cuda and tokens.dtype == torch.int32 and tokens.numel() >= max_new
        assert hidden.is_cuda and hidden.dtype == torch.float32 and hidden.is_contiguous() and hidden.shape[0] >= max_new
        stops = [c.stop_mel_token] if stop_tokens is None else list(stop_tokens)
        st = torch.tensor(stops, dtype=torch.int32, device=prompt.device) if stops else None
        torch.cuda.current_stream(prompt.device).synchronize()
        n = C.c_int32(0)
        args = (self._h, prompt.data_ptr(), prompt.shape[-2], int(max_new), st.data_ptr() if st is not None else None,
                len(stops), float(c.repeat_penalty if repeat_value is None else repeat_value),
                int(c.penalty_range if penalty_range is None else penalty_range),
                repeat_penality.data_ptr() if repeat_penality is not None else None, tokens.data_ptr(), hidden.data_ptr(),
                C.byref(n), _lib.MI_DEVICE)
        if beams > 1:
            assert tokens.is_contiguous()
            rows, mx = np.array([prompt.shape[-2]], np.int32), np.array([int(max_new)], np.int32)
            _lib.check(_lib.load().mi_gpt_generate_beam(self._h, 1, args[1], _lib.i32p(rows), _lib.i32p(mx), *args[4:9], beams,
                                                        tokens.data_ptr(), hidden.data_ptr(), int(max_new), C.byref(n), None,
                                                        _lib.MI_DEVICE), "mi_gpt_generate_beam")
        elif sampling is None:
            _lib.check(_lib.load().mi_gpt_generate(*args), "mi_gpt_generate")
        else:
            _lib.check(_lib.load().mi_gpt_generate_sampled(*args, float(sampling.temperature), int(sampling.top_k),
                                                           float(sampling.top_p), int(sampling.seed)),
                       "mi_gpt_generate_sampled")
        return int(n.value)

    def generate_batch(self, prompts, max_new, *, stop_tokens=None, repeat_value=None, penalty_range=None,
                       repeat_penality=None, sampling=None, beams: int = 1):
        """Several sentences at once (engine extension: the reference decodes one sentence at a time).  prompts = list
        of (1, P_b, hidden) graph-D outputs, max_new = list of per-sentence limits.  Every decode step streams the
        weights once for all sentences.  Returns a list of (tokens, hidden) and the (nb, mel_codes) penalty matrix.
        sampling: None (greedy), one ``Sampling`` for every sentence, or a list of nb ``Sampling`` / None (greedy item).
        beams > 1: beam search, every sentence with that many hypotheses (nb * beams <= max_batch)."""
        c = self.cfg
        nb = len(prompts)
        if _check_beams(beams, nb, c, sampling) > 1:
            res, pen = self.generate_beam(prompts, max_new, beams, stop_tokens=stop_tokens, repeat_value=repeat_value,
                                          penalty_range=penalty_range, repeat_penality=repeat_penality)
            return [(t, h) for t, h, _ in res], pen
        samp = _batch_sampling(sampling, nb)
        if nb < 1 or nb > c.max_batch or len(max_new) != nb:
            raise ValueError(f"batch of {nb} sentences; this engine was created with max_batch = {c.max_batch}")
        ps = [np.ascontiguousarray(p, dtype=np.float32).reshape(-1, c.hidden) for p in prompts]
        rows = np.ascontiguousarray([p.shape[0] for p in ps], dtype=np.int32)
        cat = np.ascontiguousarray(np.concatenate(ps, axis=0))
        mx = np.ascontiguousarray([int(m) for m in max_new], dtype=np.int32)
        cap = max(int(mx.max()), 1)
        stops = np.ascontiguousarray([c.stop_mel_token] if stop_tokens is None else list(stop_tokens), dtype=np.int32)
        pen = (np.ones((nb, c.mel_codes), np.float32) if repeat_penality is None
               else np.ascontiguousarray(repeat_penality, dtype=np.float32).reshape(nb, c.mel_codes).copy())
        toks = np.zeros((nb, cap), np.int32)
        hid = np.zeros((nb, cap, c.hidden), np.float32)
        n = np.zeros((nb,), np.int32)
        args = (self._h, nb, cat.ctypes.data, _lib.i32p(rows), _lib.i32p(mx), stops.ctypes.data if stops.size else None,
                stops.size, float(c.repeat_penalty if repeat_value is None else repeat_value),
                int(c.penalty_range if penalty_range is None else penalty_range), pen.ctypes.data, toks.ctypes.data,
                hid.ctypes.data, cap, _lib.i32p(n), _lib.MI_HOST)
        if samp is None:
            _lib.check(_lib.load().mi_gpt_generate_batch(*args), "mi_gpt_generate_batch")
        else:
            sa = _sampling_arrays(samp)
            _lib.check(_lib.load().mi_gpt_generate_batch_sampled(*args, *(a.ctypes.data for a in sa)),
                       "mi_gpt_generate_batch_sampled")
        return [(toks[b, : n[b]].copy(), hid[b, : n[b]].copy()) for b in range(nb)], pen

    def generate_queue(self, prompts, max_new, *, stop_tokens=None, repeat_value=None, penalty_range=None, sampling=None,
                       beams=None, pool: bool = False, length_penalty: float = 0.0, early_stopping: bool = False,
                       return_stats: bool = False):
        """Any number of sentences through the engine's max_batch slots (include/mi355tts.h, "sentence queue"): a slot is
        refilled as soon as its sentence stops, and the prompts admitted together run as one packed pass over the weights.
        prompts = list of (1, P_i, hidden) graph-D outputs, max_new = list of per-sentence limits.  Every sentence starts from a
        penalty vector of ones (nothing is carried between sentences: they run concurrently).  sampling: None (greedy), one
        ``Sampling`` for every sentence, or a list of n ``Sampling`` / None.  beams = B (1..8, not with sampling): beam search
        through the queue (mi_gpt_generate_queue_beam): a sentence runs as a group of B slots, the queue schedules the
        max_batch // B groups, and each result is (tokens, hidden, score) of the best hypothesis, as ``generate_beam`` gives for
        the sentence alone.  ``pool=True`` (with beams) is pool mode through the queue (mi_gpt_generate_queue_beam_pool): the
        groups run "beam search with a finished pool" with ``length_penalty`` / ``early_stopping``, ``sampling`` (one ``Sampling``
        or one per sentence) then draws the candidates, and each result is what ``generate_beam(..., pool=True)`` gives for the
        sentence alone.  Returns a list of (tokens, hidden) per sentence[, {"steps": decode steps launched, "passes": prompt
        passes}]."""
        c = self.cfg
        n = len(prompts)
        if n < 1 or len(max_new) != n:
            raise ValueError(f"{n} prompts and {len(max_new)} limits: generate_queue needs one limit per sentence, n >= 1")
        beams = _check_queue_beams(beams, c, sampling, bool(pool), length_penalty, early_stopping)
        samp = _batch_sampling(sampling, n)
        ps = [np.ascontiguousarray(p, dtype=np.float32).reshape(-1, c.hidden) for p in prompts]
        rows = np.ascontiguousarray([p.shape[0] for p in ps], dtype=np.int32)
        cat = np.ascontiguousarray(np.concatenate(ps, axis=0))
        mx = np.ascontiguousarray([int(m) for m in max_new], dtype=np.int32)
        cap = max(int(mx.max()), 1)
        stops = np.ascontiguousarray([c.stop_mel_token] if stop_tokens is None else list(stop_tokens), dtype=np.int32)
        if beams is not None:
            pm = (length_penalty, early_stopping, None if samp is None else _sampling_arrays(samp)) if pool else None
            toks, hid, cnt, sc, stats = _queue_beam_call(self._h, c, cat, rows, mx, stops,
                                                         float(c.repeat_penalty if repeat_value is None else repeat_value),
                                                         int(c.penalty_range if penalty_range is None else penalty_range), cap, beams,
                                                         pm)
            res = [(toks[i, : cnt[i]].copy(), hid[i, : cnt[i]].copy(), float(sc[i])) for i in range(n)]
            return (res, {"steps": int(stats[0]), "passes": int(stats[1])}) if return_stats else res
        sa = None if samp is None else _sampling_arrays(samp)
        toks, hid, cnt, stats = _queue_call(self._h, c, cat, rows, mx, stops,
                                            float(c.repeat_penalty if repeat_value is None else repeat_value),
                                            int(c.penalty_range if penalty_range is None else penalty_range), cap, sa)
        res = [(toks[i, : cnt[i]].copy(), hid[i, : cnt[i]].copy()) for i in range(n)]
        return (res, {"steps": int(stats[0]), "passes": int(stats[1])}) if return_stats else res

    def queue_session(self, prompts, max_new, *, stop_tokens=None, repeat_value=None, penalty_range=None, sampling=None,
                      beams=None, pool: bool = False, length_penalty: float = 0.0, early_stopping: bool = False,
                      device: bool = False) -> QueueSession:
        """``generate_queue`` as a session that hands out rows as they appear: arguments as there; returns a ``QueueSession``
        (a context manager) whose ``advance()`` runs one round.  device=True keeps tokens / hidden as torch tensors on the
        engine's device (``BigVGANVocoder.run_latent_windows_torch`` reads the rows where they lie).  beams = B: beam search, a
        sentence's tokens, rows and score (``QueueSession.scores``) appearing all at once when it is retired; pool / length_penalty
        / early_stopping (and sampling with them) as in ``generate_queue``.  While the session is open
        the other decode entries of this engine raise (MI_ESTATE)."""
        c = self.cfg
        n = len(prompts)
        if n < 1 or len(max_new) != n:
            raise ValueError(f"{n} prompts and {len(max_new)} limits: queue_session needs one limit per sentence, n >= 1")
        beams = _check_queue_beams(beams, c, sampling, bool(pool), length_penalty, early_stopping)
        samp = _batch_sampling(sampling, n)
        ps = [np.ascontiguousarray(p, dtype=np.float32).reshape(-1, c.hidden) for p in prompts]
        rows = np.ascontiguousarray([p.shape[0] for p in ps], dtype=np.int32)
        cat = np.ascontiguousarray(np.concatenate(ps, axis=0))
        mx = np.ascontiguousarray([int(m) for m in max_new], dtype=np.int32)
        cap = max(int(mx.max()), 1)
        stops = np.ascontiguousarray([c.stop_mel_token] if stop_tokens is None else list(stop_tokens), dtype=np.int32)
        sa = None if samp is None else _sampling_arrays(samp)
        return QueueSession(self, cat, rows, mx, stops, float(c.repeat_penalty if repeat_value is None else repeat_value),
                            int(c.penalty_range if penalty_range is None else penalty_range), cap, sa, device, beams,
                            (length_penalty, early_stopping) if pool else None)

    def generate_batch_torch(self, prompts_cat, prompt_rows, max_new, tokens, hidden, *, stop_tokens=None,
                             repeat_value=None, penalty_range=None, sampling=None, beams: int = 1):
        """Device-resident variant: prompts_cat (sum P_b, hidden) float32 CUDA tensor; tokens (nb, cap) int32 and hidden
        (nb, cap, hidden) float32 CUDA tensors are filled.  Returns the per-sentence token counts."""
        import torch
        c = self.cfg
        nb = len(prompt_rows)
        beams = _check_beams(beams, nb, c, sampling)
        assert prompts_cat.is_cuda and prompts_cat.dtype == torch.float32 and prompts_cat.is_contiguous()
        assert tokens.is_cuda and tokens.dtype == torch.int32 and tokens.is_contiguous() and tokens.shape[0] == nb
        assert hidden.is_cuda and hidden.dtype == torch.float32 and hidden.is_contiguous() and hidden.shape[:2] == tokens.shape
        rows = np.ascontiguousarray(prompt_rows, dtype=np.int32)
        mx = np.ascontiguousarray(max_new, dtype=np.int32)
        stops = [c.stop_mel_token] if stop_tokens is None else list(stop_tokens)
        st = torch.tensor(stops, dtype=torch.int32, device=prompts_cat.device) if stops else None
        torch.cuda.current_stream(prompts_cat.device).synchronize()
        n = np.zeros((nb,), np.int32)
        samp = _batch_sampling(sampling, nb)
        args = (self._h, nb, prompts_cat.data_ptr(), _lib.i32p(rows), _lib.i32p(mx), st.data_ptr() if st is not None else None,
                len(stops), float(c.repeat_penalty if repeat_value is None else repeat_value),
                int(c.penalty_range if penalty_range is None else penalty_range), None, tokens.data_ptr(), hidden.data_ptr(),
                int(tokens.shape[1]), _lib.i32p(n), _lib.MI_DEVICE)
        if beams > 1:
            _lib.check(_lib.load().mi_gpt_generate_beam(*args[:10], beams, *args[10:14], None, _lib.MI_DEVICE),
                       "mi_gpt_generate_beam")
        elif samp is None:
            _lib.check(_lib.load().mi_gpt_generate_batch(*args), "mi_gpt_generate_batch")
        else:
            sa = _sampling_arrays(samp)
            _lib.check(_lib.load().mi_gpt_generate_batch_sampled(*args, *(a.ctypes.data for a in sa)),
                       "mi_gpt_generate_batch_sampled")
        return n

    def generate_beam(self, prompts, max_new, beams: int, *, stop_tokens=None, repeat_value=None, penalty_range=None,
                      repeat_penality=None, pool: bool = False, length_penalty: float = 0.0, early_stopping: bool = False,
                      sampling=None):
        """Beam search (include/mi355tts.h, "beam search"; always the beam entry, beams = 1 included): every sentence runs
        ``beams`` hypotheses over one shared KV cache and its best one is returned.  prompts / max_new as generate_batch.
        Returns a list of (tokens, hidden, score) — score = the hypothesis' cumulative log-probability — and the
        (nb, mel_codes) penalty matrix.

        ``pool=True`` is the second beam mode ("beam search with a finished pool"): finished hypotheses are kept aside, the
        best of the pool is returned (score = its cumulative log-probability / length ** length_penalty), and with
        ``sampling`` (one Sampling or a list of nb) the candidates are drawn.  The penalty matrix is then returned as given."""
        c = self.cfg
        nb = len(prompts)
        if not pool and (length_penalty != 0.0 or early_stopping):
            raise ValueError("length_penalty and early_stopping belong to pool=True")
        samp = _batch_sampling(sampling, nb)
        if samp is not None and not pool:
            raise ValueError("beams and sampling do not combine without pool=True: that beam search is deterministic")
        beams = _check_beams(beams, nb, c, sampling=samp, pool=bool(pool))
        if nb < 1 or nb * beams > c.max_batch or len(max_new) != nb:
            raise ValueError(f"{nb} sentences x {beams} beams; this engine was created with max_batch = {c.max_batch}")
        if samp is not None and any(x is None for x in samp):
            raise ValueError("pool mode samples every sentence of the call or none")
        ps = [np.ascontiguousarray(p, dtype=np.float32).reshape(-1, c.hidden) for p in prompts]
        rows = np.ascontiguousarray([p.shape[0] for p in ps], dtype=np.int32)
        cat = np.ascontiguousarray(np.concatenate(ps, axis=0))
        mx = np.ascontiguousarray([int(m) for m in max_new], dtype=np.int32)
        cap = max(int(mx.max()), 1)
        stops = np.ascontiguousarray([c.stop_mel_token] if stop_tokens is None else list(stop_tokens), dtype=np.int32)
        pen = (np.ones((nb, c.mel_codes), np.float32) if repeat_penality is None
               else np.ascontiguousarray(repeat_penality, dtype=np.float32).reshape(nb, c.mel_codes).copy())
        toks = np.zeros((nb, cap), np.int32)
        hid = np.zeros((nb, cap, c.hidden), np.float32)
        n = np.zeros((nb,), np.int32)
        sc = np.zeros((nb,), np.float32)
        head = (self._h, nb, cat.ctypes.data, _lib.i32p(rows), _lib.i32p(mx), stops.ctypes.data if stops.size else None, stops.size,
                float(c.repeat_penalty if repeat_value is None else repeat_value),
                int(c.penalty_range if penalty_range is None else penalty_range), pen.ctypes.data, beams)
        tail = (toks.ctypes.data, hid.ctypes.data, cap, _lib.i32p(n), sc.ctypes.data, _lib.MI_HOST)
        if pool:
            sa = None if samp is None else _sampling_arrays(samp)
            _lib.check(_lib.load().mi_gpt_generate_beam_pool(
                *head, float(length_penalty), int(early_stopping), *((None,) * 4 if sa is None else (a.ctypes.data for a in sa)),
                *tail), "mi_gpt_generate_beam_pool")
        else:
            _lib.check(_lib.load().mi_gpt_generate_beam(*head, *tail), "mi_gpt_generate_beam")
        return [(toks[b, : n[b]].copy(), hid[b, : n[b]].copy(), float(sc[b])) for b in range(nb)], pen

    def generate(self, conds_latent, text_ids, *, max_generate_length=None, **kw):
        """Inference_IndexTTS_ONNX.py:723-783 for one sentence: B, C, D then E until a stop token or
        MAX_GENERATE_LENGTH - concat_len tokens.  Returns (tokens, save_last_hidden_state (n, hidden), penalty).
        ``sampling=Sampling(...)`` (passed on to generate_from_prompt) draws the tokens, ``beams=N`` runs beam search; the
        default is greedy."""
        c = self.cfg
        text_h = self.text_embed(text_ids)
        mel_h, _ = self.mel_embed(c.start_mel_token, 0)
        prompt, concat_len = self.concat(np.asarray(conds_latent, np.float32), text_h, mel_h)
        limit = (c.max_generate_length if max_generate_length is None else int(max_generate_length)) - int(concat_len[0])
        return self.generate_from_prompt(prompt, limit, **kw)


class IndexCond:
    """IndexTTS graph A (ort_session_A of Inference_IndexTTS_ONNX.py:700-712; IndexTTS_A, Export_IndexTTS.py:74-200): int16
    prompt audio -> (conds_latent, vocoder conditioning).  ``state``: upstream-named tensors of weights.cond_spec (folds applied
    here), or ``blob``: the packed array of weights.pack_cond."""

    def __init__(self, cfg, state=None, blob=None, device: int = 0):
        from .config import IndexCondConfig
        from . import weights as W
        assert isinstance(cfg, IndexCondConfig)
        self.cfg = cfg
        _lib.init(device)
        if blob is None:
            if state is None:
                raise ValueError("IndexCond needs a state dict or a packed blob")
            blob = W.pack_cond(cfg, state)
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        arr = np.asarray(cfg.to_int_array(), dtype=np.int32)
        L = _lib.load()
        n = L.mi_indextts_cond_param_count(_lib.i32p(arr), arr.size)
        if n != blob.size:
            raise ValueError(f"IndexCond: blob has {blob.size} weights, the config needs {n}")
        self._h = L.mi_indextts_cond_create(_lib.i32p(arr), arr.size, blob.ctypes.data_as(C.POINTER(C.c_float)), blob.size, device)
        if not self._h:
            raise _lib.MiError("mi_indextts_cond_create: " + L.mi_last_error().decode())
        self.ncond = cfg.voc_initial + sum(cfg.voc_channels)

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().mi_indextts_cond_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, audio, return_mel: bool = False):
        """audio int16 (L,) or (1, 1, L) -> (conds (ncond,) = cond_layer | conds_0 | ..., conds_latent (latents, model_dim)[, mel])."""
        a = np.ascontiguousarray(np.asarray(audio).reshape(-1))
        if a.dtype != np.int16:
            raise ValueError("audio must be int16")
        cfg = self.cfg
        conds = np.empty((self.ncond,), np.float32)
        lat = np.empty((cfg.latents, cfg.model_dim), np.float32)
        mel = np.empty((cfg.frames(a.size), cfg.n_mels), np.float32) if return_mel else None
        _lib.check(_lib.load().mi_indextts_cond_run(self._h, a.ctypes.data, a.size, conds.ctypes.data, lat.ctypes.data,
                                                    None if mel is None else mel.ctypes.data, _lib.MI_HOST), "mi_indextts_cond_run")
        return (conds, lat, mel) if return_mel else (conds, lat)

    def split_conds(self, conds):
        """The graph's separate outputs: (save_bigvgan_conds_0..n-1 each (1, C_i, 1), bigvgan_cond_layer_speaker_embedding (1, C0, 1))."""
        cfg = self.cfg
        o = cfg.voc_initial
        outs = []
        for ch in cfg.voc_channels:
            outs.append(conds[o:o + ch].reshape(1, ch, 1)); o += ch
        return outs, conds[:cfg.voc_initial].reshape(1, cfg.voc_initial, 1)
