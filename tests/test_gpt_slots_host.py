"""CPU: more than 16 batch slots on the host side — the queue's scheduling model (mi355tts.indextts.queue_schedule) with 17..64
slots, held to the properties tests/test_gpt_queue_schedule.py holds it to below 17, and the example's argument parser."""
import importlib.util
import math
import os

import numpy as np
import pytest

from mi355tts.indextts import lockstep_steps, queue_schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("seed", range(12))
def test_schedule_properties_above_16_slots(seed):
    """Even seeds: no early stop (lengths == max_new); odd seeds: every sentence stops somewhere up to its limit.  The step
    bounds are those of test_schedule_properties: the lock-step count without early stops, the lock-step count of sentences
    15 tokens longer with them (a stop is seen at the end of a run of up to 16 steps)."""
    rng = np.random.default_rng(2000 + seed)
    slots = int(rng.integers(17, 65))
    n = int(rng.integers(1, 160))
    max_seq = int(rng.integers(64, 1100))
    rows = rng.integers(1, 64, n).tolist()
    limit = rng.integers(0, 70, n).tolist()
    if seed % 3 == 0:
        limit[int(rng.integers(0, n))] = 0
    lens = list(limit) if seed % 2 == 0 else [0 if m == 0 else int(rng.integers(1, m + 1)) for m in limit]
    steps, passes = queue_schedule(rows, limit, lens, slots, max_seq)
    admitted = [i for p in passes for i, _ in p]
    assert sorted(admitted) == [i for i in range(n) if limit[i] > 0]            # exactly once, and only those with a limit
    assert admitted == sorted(admitted)                                           # index order
    for p in passes:
        assert p and len({s for _, s in p}) == len(p) and len(p) <= slots         # one sentence per slot in a pass
        assert all(0 <= s < min(slots, n) for _, s in p)
        assert len(p) == 1 or sum(rows[i] for i, _ in p) <= max_seq               # the scratch bound (a lone sentence always fits)
    last_in_slot = {}
    for p in passes:
        for i, s in p:
            assert s not in last_in_slot or last_in_slot[s] < i                   # a slot is reused only by a later sentence
            last_in_slot[s] = i
    longest = max(lens) if lens else 0
    assert steps >= math.ceil(max(longest - 1, 0))
    if seed % 2 == 0:
        assert steps <= lockstep_steps(lens, slots)
    else:
        assert steps <= lockstep_steps([x + 15 if x else 0 for x in lens], slots)


def test_first_pass_fills_more_than_16_slots():
    steps, passes = queue_schedule([10] * 70, [5] * 70, [5] * 70, 64, 1024)
    assert [len(p) for p in passes] == [64, 6] and [s for _, s in passes[0]] == list(range(64))
    assert steps == 8
    # the packed-row capacity splits a pass, whatever the slot count: 64 slots, 20 rows each, 96 rows of scratch
    _, passes = queue_schedule([20] * 30, [3] * 30, [3] * 30, 64, 96)
    assert [len(p) for p in passes] == [4] * 7 + [2]


@pytest.fixture(scope="module")
def example():
    spec = importlib.util.spec_from_file_location("indextts_infer_example", os.path.join(ROOT, "examples", "indextts_infer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_parser_takes_64_slots(example):
    a = example.parse_args(["--queue", "--slots", "64"])
    assert a.queue and a.slots == 64
    a = example.parse_args(["--takes", "64"])
    assert a.takes == 64 and a.sampled
    assert example.parse_args(["--num-beams", "8"]).num_beams == 8
    for bad in (["--queue", "--slots", "65"], ["--takes", "65"], ["--slots", "0"], ["--num-beams", "9"]):
        with pytest.raises(SystemExit):
            example.parse_args(bad)
