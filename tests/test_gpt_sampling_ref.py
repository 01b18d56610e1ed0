"""CPU: the float64 reference of the IndexTTS GPT sampler (tests/gpt_sampling_ref.py) that the GPU tests measure against, the
Python-side parameter record, and the cases the GPU tests share (none of them borderline for the reference itself)."""
import numpy as np
import pytest

import gpt_sampling_ref as R
from mi355tts.indextts import Sampling


def test_philox4x32_10_known_answers():
    """the known-answer vectors published with Random123 (kat_vectors, philox4x32 10 rounds)"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, out in kat:
        assert tuple(R.philox4x32_10(ctr, key)) == out
    u = R.uniform(0, 0)
    assert u.dtype == np.float32 and float(u) == (0x6627e8d5 >> 8) * 2.0 ** -24 and 0.0 <= float(u) < 1.0
    assert R.uniform(5, 3) != R.uniform(5, 4) and R.uniform(5, 3) != R.uniform(6, 3) and R.uniform((1 << 32) + 5, 3) != R.uniform(5, 3)


@pytest.fixture(scope="module")
def row():
    rng = np.random.default_rng(3)
    lg = (rng.standard_normal(301) * 2.5).astype(np.float32)
    pen = np.where(rng.random(301) < 0.2, np.float32(0.7), np.float32(1.0))
    return lg, pen


def test_z_is_float32_and_penalty_quirk(row):
    lg, pen = row
    z = R.z32(lg, pen, 0.7)
    assert z.dtype == np.float32
    inv_t = np.float32(1.0) / np.float32(0.7)
    np.testing.assert_array_equal(z, (lg * pen) * inv_t)
    neg = (lg < 0) & (pen < 1)
    assert neg.any() and (z[neg] > (lg[neg] * inv_t)).all()          # a penalised negative logit moves UP, like the reference


def test_reference_properties(row):
    lg, pen = row
    for n in range(8):
        g = R.sample(lg, pen, 1.3, 1, 0.4, 9, n)
        assert g["token"] == int(np.argmax(lg * pen)) and g["P"].sum() == 1 and g["margin"] == np.inf
        a = R.sample(lg, pen, 1.0, 0, 1.0, 9, n)
        assert a["K"].all() and a["P"].all() and abs(a["probs"].sum() - 1) < 1e-12
        for k, p, t in ((30, 0.8, 1.0), (5, 0.3, 0.7), (300, 0.95, 1.5), (0, 0.05, 1.0), (400, 1.0, 1.0)):
            r = R.sample(lg, pen, t, k, p, 9, n)
            z = R.z32(lg, pen, t)
            assert not (r["P"] & ~r["K"]).any()                                 # P is a subset of K
            assert r["P"][int(np.argmax(z))] and r["P"][r["token"]]              # the argmax is kept; the token is in P
            assert r["K"].sum() >= (k if 0 < k < lg.size else lg.size)
            assert z[r["K"]].min() > (z[~r["K"]].max() if (~r["K"]).any() else -np.inf)
            assert z[r["P"]].min() > (z[~r["P"]].max() if (~r["P"]).any() else -np.inf)
            assert abs(r["probs"].sum() - 1) < 1e-12 and (r["probs"][~r["P"]] == 0).all()
            full = np.where(r["K"], np.exp(z.astype(np.float64) - z.max()), 0)
            assert full[r["P"]].sum() >= float(np.float32(p)) * full.sum() * (1 - 1e-12)
            if r["P"].sum() > 1:                                                 # ... and no smaller prefix reaches it
                drop = r["P"] & (z > z[r["P"]].min())
                assert full[drop].sum() < float(np.float32(p)) * full.sum()


def test_ties_are_closed():
    tr = R.tie_row()
    r = R.sample(tr, None, 1.0, 30, 0.8, 5, 3)
    assert r["K"].sum() > 30                                  # ties at t_k are all kept
    for s in (r["K"], r["P"]):
        assert not np.isin(tr[~s], tr[s]).any()               # no value is split between in and out
    assert 1 < r["P"].sum() < r["K"].sum() and r["margin"] > 1e-4
    r1 = R.sample(tr, None, 1.0, 30, 1.0, 5, 3)
    np.testing.assert_array_equal(r1["P"], r1["K"])


def test_reference_frequencies():
    """4096 positions on the fixed row: every code of P within 5 binomial standard deviations (deterministic given FREQ_SEED)"""
    lg = R.freq_row()
    ref = R.sample(lg, None, 1.0, 30, 0.8, R.FREQ_SEED, 0)
    toks = [R.sample(lg, None, 1.0, 30, 0.8, R.FREQ_SEED, n)["token"] for n in range(R.FREQ_N)]
    assert 5 < ref["P"].sum() <= 30 and R.freq_ok(toks, ref)
    assert not R.freq_ok([int(np.argmax(lg))] * R.FREQ_N, ref)          # the check has teeth


@pytest.mark.parametrize("codes", R.CODES)
def test_shared_cases_are_not_borderline(codes):
    """The GPU test demands token equality wherever the margin is >= 1e-5; the committed rows and seeds leave the reference
    itself no borderline case at 1e-4."""
    c = R.cases(codes)
    assert c["logits"].shape == (R.ROWS, codes) and ((c["pen"] < 1) & (c["logits"] < 0)).any()
    assert len(c["refs"]) == 6 * 4 * 3
    for (k, p, t), (seeds, pos, refs) in c["refs"].items():
        assert len(refs) == R.ROWS and min(r["margin"] for r in refs) >= 1e-4
        for r in range(0, R.ROWS, 5):                                    # the stored results are what `sample` gives
            again = R.sample(c["logits"][r], c["pen"][r], t, k, p, int(seeds[r]), int(pos[r]))
            assert again["token"] == refs[r]["token"] and again["u"] == refs[r]["u"]


def test_bookkeeping_matches_the_driver_loop():
    before, pen = R.bookkeeping([3, 4, 3, 5, 6, 7], 10, 0.7, 2, stop_tokens=[7])
    assert len(before) == 6 and (before[0] == 1).all()
    exp = np.ones(10, np.float32)
    exp[[5, 6]] = 0.7                 # 3 and 4 were released again two tokens later; the stop token is not penalised
    exp[3] = 1.0
    np.testing.assert_array_equal(pen, exp)


def test_sampling_dataclass_validates():
    s = Sampling()
    assert (s.temperature, s.top_k, s.top_p, s.seed) == (1.0, 30, 0.8, 0)
    Sampling(0.5, 0, 1.0, 2 ** 64 - 1)
    for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=float("inf")),
                dict(top_k=-1), dict(top_k=1.5), dict(top_p=0.0), dict(top_p=1.01), dict(top_p=float("nan")),
                dict(seed=-1), dict(seed=2 ** 64)):
        with pytest.raises(ValueError):
            Sampling(**bad)
    with pytest.raises(Exception):
        s.top_k = 3                                            # frozen: one record, one take
