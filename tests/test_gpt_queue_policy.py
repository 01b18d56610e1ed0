"""CPU: the library's own scheduling policy (mi::QueuePolicy, csrc/gpt_queue.h, the object GptQueue::round() drives on the device)
against its readable statement, mi355tts.indextts.queue_schedule.  mi_gpt_queue_schedule drives that object on the host alone:
the prompt pass gives token 0 and a unit is done when its sentence holds lengths[i] tokens, which is what the device states tell
the engine.  Equality is exact, on integers: the step count and every (sentence, unit) of every pass."""
import ctypes as C

import numpy as np
import pytest

from mi355tts import _lib
from mi355tts.indextts import queue_schedule
from test_gpt_queue_beam_host import ALL, _random_case

BEAMS = (1, 2, 3, 5, 8)
MORE = [_random_case(seed) for seed in range(12, 212)]

# (case, what queue_schedule gives, checked by hand)
PINNED = [
    (([7], [5], [3], 4, 64), (4, [[(0, 0)]])),                                       # n = 1: one unit, one run to the limit
    (([5, 6, 7], [0, 0, 0], [0, 0, 0], 2, 64), (0, [])),                             # every max_new == 0: nothing is admitted
    (([64], [1], [1], 2, 64), (0, [[(0, 0)]])),                                      # a lone prompt of exactly max_seq rows
    (([64, 3], [1, 2], [1, 2], 2, 64), (1, [[(0, 0)], [(1, 1)]])),                   # ... and nothing shares its pass
    (([40, 30, 10], [3, 3, 3], [3, 3, 3], 3, 64), (2, [[(0, 0)], [(1, 1), (2, 2)]])),  # a pass cut by max_seq at its second sentence
]


def _arr(x):
    return None if x is None else np.ascontiguousarray(x, dtype=np.int32)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def native(rows, limit, lens, slots, max_seq, beams=1, n=None):
    """-> (rc, steps, passes) with passes rebuilt from pass_of / unit_of (index order inside a pass)"""
    n = len(rows) if n is None else n
    r, m, l = _arr(rows), _arr(limit), _arr(lens)
    steps, n_passes = C.c_int32(-1), C.c_int32(-1)
    pass_of, unit_of = np.full(max(n, 1), -2, np.int32), np.full(max(n, 1), -2, np.int32)
    rc = _lib.load().mi_gpt_queue_schedule(n, _ptr(r), _ptr(m), _ptr(l), slots, max_seq, beams, C.byref(steps), C.byref(n_passes),
                                           _ptr(pass_of), _ptr(unit_of))
    if rc != 0:
        return rc, None, None
    passes = [[] for _ in range(n_passes.value)]
    for i in range(n):
        assert (pass_of[i] < 0) == (limit[i] == 0) and (unit_of[i] < 0) == (limit[i] == 0), i
        if pass_of[i] >= 0:
            passes[pass_of[i]].append((i, int(unit_of[i])))
    return rc, steps.value, passes


def _sweep(case, model_per_spare=True):
    """model_per_spare off: the model is asked once per beams (that it ignores the spare slots is test_beams_divide_the_slots)"""
    rows, limit, lens, groups, max_seq = case
    for beams in BEAMS:
        for spare in range(beams):                      # slots that do not fill a unit are never scheduled
            slots = groups * beams + spare
            if model_per_spare or spare == 0:
                want = queue_schedule(rows, limit, lens, slots, max_seq, beams=beams)
            assert native(rows, limit, lens, slots, max_seq, beams) == (0,) + want, (case, beams, spare)


@pytest.mark.parametrize("k", range(len(ALL)))
def test_entry_equals_the_host_model(k):
    """the six hand-checked and the twelve seeded cases of tests/test_gpt_queue_beam_host.py, over every beams and spare"""
    _sweep(ALL[k])


def test_entry_equals_the_host_model_on_200_more_seeds():
    for case in MORE:
        _sweep(case, model_per_spare=False)


@pytest.mark.parametrize("k", range(len(PINNED)))
def test_pinned_shapes(k):
    case, want = PINNED[k]
    assert queue_schedule(*case) == want
    assert native(*case) == (0,) + want
    _sweep(case)


def test_rejected_arguments_return_einval():
    """the argument sets tests/test_gpt_queue_schedule.py and tests/test_gpt_queue_beam_host.py hold queue_schedule to"""
    for rows, limit, lens, slots, max_seq, beams in [
        ([5], [3], [4], 2, 64, 1),              # produced more than the limit
        ([5], [3], [0], 2, 64, 1),              # a sentence with a limit produces at least its token 0
        ([5], [3], [3], 2, 64, 3),              # not one whole group
        ([5], [3], [3], 2, 64, 0),
    ]:
        with pytest.raises(ValueError):
            queue_schedule(rows, limit, lens, slots, max_seq, beams=beams)
        assert native(rows, limit, lens, slots, max_seq, beams)[0] == _lib.MI_EINVAL
    # arrays that disagree in length: the C ABI has one n, and a caller with no entry per sentence has no array to give
    with pytest.raises(ValueError):
        queue_schedule([5, 5], [3], [3], 2, 64)
    assert native([5, 5], None, None, 2, 64, n=2)[0] == _lib.MI_EINVAL
    assert native([], [], [], 2, 64)[0] == _lib.MI_EINVAL
    assert b"mi_gpt_queue_schedule" in _lib.load().mi_last_error()
