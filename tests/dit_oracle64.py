"""The DiT evaluation of the numpy oracle carried out in float64, and the two error gates the DiT tests apply against it.

oracle/f5_np.py computes in whatever its module global F32 names; with F32 = float64 (set through pytest's monkeypatch, so the
oracle itself keeps computing what the fixtures pin) and float64 weights and inputs, dit_forward is the same function without
the fp32 rounding of every intermediate.  The rotary tables keep their fp16 rounding (part of the model): they are built in
fp32 first and only then widened.  The fp32 oracle's own error against it is ~5e-7 rel RMS at mid width, a third of what the
fp32 engine achieves, which is why the engine's gates are taken against this one (tests/test_oracle_f5.py pins it).
"""
import numpy as np

from oracle import f5_np as O


def rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))


def widen(st):
    """The (folded) state dict with every floating-point array as float64."""
    return {k: (v.astype(np.float64) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v) for k, v in st.items()}


def rope64(N, dim_head, shift_from=None):
    """O.rope_tables in fp32 (fp16-rounded values), widened.  shift_from = p: positions p .. N-1 take the angles of p+1 .. N
    (a RoPE off by one on the last rows: the gate-sensitivity test's injected bug)."""
    cos, sin = O.rope_tables(N + 1, dim_head)
    idx = np.arange(N)
    if shift_from is not None:
        idx[shift_from:] += 1
    return cos[idx].astype(np.float64), sin[idx].astype(np.float64)


def dit_forward64(monkeypatch, cfg, st64, x, cond, cond_drop, t_emb, cos=None, sin=None):
    """O.dit_forward in float64 -> (2, N, mel).  st64 = widen(st); t_emb from the fp32 O.time_tables (what the engines use)."""
    if cos is None:
        cos, sin = rope64(x.shape[0], cfg.dim_head)
    f = lambda a: np.asarray(a, dtype=np.float64)
    with monkeypatch.context() as m:
        m.setattr(O, "F32", np.float64)
        return O.dit_forward(cfg, st64, f(x), f(cond), f(cond_drop), f(t_emb), f(cos), f(sin))


def dit_errors(got, ref):
    """(overall rel RMS, worst row) of got against ref, both (..., mel); a row is one token of one batch item and its error is
    rms(row error) / rms(ref): a bug confined to one row group — the last, partial one of a tiling above all — is averaged
    away by the overall figure (58 rows of 2074 weigh 1/6 of their own error) but not by the row figure."""
    d = np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64)
    scale = rms(ref)
    rows = np.sqrt(np.mean(np.square(d.reshape(-1, d.shape[-1])), axis=-1))
    return rms(d) / scale, float(rows.max()) / scale


# fp32 engines at mid width (dim 1024) against dit_forward64 — tests/test_gpu_dit_tilings.py
# (achieved over its grid: 1.24e-6 overall, 1.83e-6 worst row; the gates are about 3x that)
F32_OVERALL_GATE = 3.5e-6
F32_ROW_GATE = 5e-6


def dit_gate_failures(got, ref, overall=F32_OVERALL_GATE, row=F32_ROW_GATE):
    """The gates that got trips against ref: a subset of {"overall", "row"}, and the two errors."""
    e_all, e_row = dit_errors(got, ref)
    bad = set()
    if not e_all <= overall:
        bad.add("overall")
    if not e_row <= row:
        bad.add("row")
    return bad, e_all, e_row
