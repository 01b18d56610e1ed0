"""CPU: the host side of beam search through the sentence queue.  With beams the queue schedules groups of B slots, so its host
model is ``queue_schedule`` over ``slots // B`` units (include/mi355tts.h, "beam search through the sentence queue"); the
``beams`` keyword does that division.  The cases are those of tests/test_gpt_queue_schedule.py.  And the two C-ABI entries exist."""
import numpy as np
import pytest

from mi355tts import _lib
from mi355tts.indextts import queue_schedule

# (prompt_rows, max_new, lengths, slots, max_seq): the hand-checked cases of tests/test_gpt_queue_schedule.py
CASES = [
    ([10] * 5, [65, 17, 17, 17, 17], [65, 17, 17, 17, 17], 2, 96),
    ([10] * 6, [40] * 6, [40, 3, 1, 25, 40, 9], 3, 96),
    ([60, 50, 10, 5], [4] * 4, [4] * 4, 4, 96),
    ([5, 5, 5], [3, 0, 3], [3, 0, 3], 2, 64),
    ([5], [0], [0], 4, 64),
    ([8] * 10, [10, 59, 32, 18, 21, 31, 1, 46, 2, 68], [4, 22, 29, 5, 1, 21, 1, 23, 1, 49], 12, 1024),
]


def _random_case(seed):
    """the generator of test_schedule_properties"""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(1, 40))
    slots = int(rng.integers(1, 17))
    max_seq = int(rng.integers(64, 400))
    rows = rng.integers(1, 64, n).tolist()
    limit = rng.integers(0, 70, n).tolist()
    if seed % 3 == 0:
        limit[int(rng.integers(0, n))] = 0
    lens = list(limit) if seed % 2 == 0 else [0 if m == 0 else int(rng.integers(1, m + 1)) for m in limit]
    return rows, limit, lens, slots, max_seq


ALL = CASES + [_random_case(seed) for seed in range(12)]


@pytest.mark.parametrize("beams", [1, 2, 3, 5, 8])
def test_beams_divide_the_slots(beams):
    for rows, limit, lens, groups, max_seq in ALL:
        want = queue_schedule(rows, limit, lens, groups, max_seq)
        for spare in range(beams):                      # slots that do not fill a group are never run
            assert queue_schedule(rows, limit, lens, groups * beams + spare, max_seq, beams=beams) == want


def test_one_beam_is_the_old_result():
    assert queue_schedule([10] * 5, [65, 17, 17, 17, 17], [65, 17, 17, 17, 17], 2, 96, beams=1) == \
        (64, [[(0, 0), (1, 1)], [(2, 1)], [(3, 1)], [(4, 1)]])
    for rows, limit, lens, slots, max_seq in ALL:
        assert queue_schedule(rows, limit, lens, slots, max_seq, beams=1) == queue_schedule(rows, limit, lens, slots, max_seq)


def test_beams_that_do_not_fit_are_rejected():
    with pytest.raises(ValueError):
        queue_schedule([5], [3], [3], 2, 64, beams=3)       # not one whole group
    with pytest.raises(ValueError):
        queue_schedule([5], [3], [3], 2, 64, beams=0)


def test_the_two_entries_are_exported():
    L = _lib.load()
    for name in ("mi_gpt_generate_queue_beam", "mi_gpt_queue_begin_beam"):
        assert hasattr(L, name), f"{name} is not exported"
        assert getattr(L, name).argtypes is not None
