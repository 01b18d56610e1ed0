"""CPU: the host side of pool-mode beam search through the sentence queue (include/mi355tts.h, "pool mode through the sentence
queue"): the two C-ABI entries exist with their prototypes, the Python argument errors are raised before any library call that
needs a device, and the schedule's host model takes the SELECTIONS a sentence ran as its length (in pool mode the length a
sentence returns is pool entry 0's, which the schedule never sees)."""
from types import SimpleNamespace

import numpy as np
import pytest

from mi355tts import _lib
from mi355tts.config import IndexGPTConfig
from mi355tts.indextts import IndexGPT, Sampling, queue_schedule

# the eight sentences of tests/test_gpu_gpt_queue_beam_pool.py: prompt rows (4 conditioning rows, TEXT[b] + 2 text rows, the start
# code), limits, and the selections each ran at 3 beams, deterministic, length_penalty 0, stop id 3 (float64 oracle)
TEXT = (6, 3, 9, 5, 1, 8, 4, 7)
ROWS = [4 + t + 2 + 1 for t in TEXT]
LIMITS = [14, 9, 11, 3, 12, 1, 10, 6]
SELECTIONS = [7, 9, 4, 3, 7, 1, 9, 6]
RETURNED = [3, 7, 1, 3, 1, 1, 3, 3]


def test_the_two_entries_are_exported():
    L = _lib.load()
    for name, nargs in (("mi_gpt_generate_queue_beam_pool", 23), ("mi_gpt_queue_begin_beam_pool", 21)):
        assert hasattr(L, name), f"{name} is not exported"
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == nargs


def _no_device():
    """an IndexGPT that has no handle: a call that got as far as the library would fail on it, not raise ValueError"""
    cfg = IndexGPTConfig.small()
    return SimpleNamespace(cfg=IndexGPTConfig(**{**cfg.__dict__, "max_batch": 7}), _h=None), cfg


@pytest.mark.parametrize("entry", [IndexGPT.generate_queue, IndexGPT.queue_session])
def test_argument_errors_come_before_the_library(entry):
    fake, cfg = _no_device()
    prompts = [np.zeros((1, 5, cfg.hidden), np.float32)] * 3
    limits = [4, 4, 4]
    sp = Sampling(1.0, 30, 0.8, 5)
    with pytest.raises(ValueError, match="beams"):
        entry(fake, prompts, limits, pool=True)                               # pool mode is a beam mode
    with pytest.raises(ValueError, match="beams"):
        entry(fake, prompts, limits, pool=True, sampling=sp)
    with pytest.raises(ValueError, match="pool"):
        entry(fake, prompts, limits, beams=3, sampling=sp)                    # sampling with beams needs the pool
    with pytest.raises(ValueError, match="pool"):
        entry(fake, prompts, limits, beams=3, length_penalty=1.0)
    with pytest.raises(ValueError, match="pool"):
        entry(fake, prompts, limits, beams=3, early_stopping=True)
    with pytest.raises(ValueError):
        entry(fake, prompts, limits, beams=3, pool=True, sampling=[sp, None, sp])     # every sentence sampled, or none
    with pytest.raises(ValueError):
        entry(fake, prompts, limits, beams=8, pool=True)                      # one group does not fit max_batch = 7
    with pytest.raises(ValueError):
        entry(fake, prompts, limits, beams=0, pool=True)


def test_schedule_counts_selections_not_returned_lengths():
    """two groups of 3 beams in 7 slots (one slot never run), by hand: pass 0 admits 0 and 1 and both end inside the first run of 8
    steps (nearest limit 9); 2 and 3, a run of 2 (limit 3) retires 3; 4 takes group 1, a run of 8 ends 2 and 4; 5 and 6, where 5
    (limit 1) is done after its pass and 7 takes its group at once; runs of 5 and 4 end 7 and 6"""
    assert hasattr(_lib.load(), "mi_gpt_generate_queue_beam_pool")        # the entry whose stats this models
    steps, passes = queue_schedule(ROWS, LIMITS, SELECTIONS, 7, 64, beams=3)
    assert steps == 8 + 2 + 8 + 5 + 4
    assert passes == [[(0, 0), (1, 1)], [(2, 0), (3, 1)], [(4, 1)], [(5, 0), (6, 1)], [(7, 0)]]
    # the lengths the sentences return describe another schedule: not what the entry's stats report
    assert queue_schedule(ROWS, LIMITS, RETURNED, 7, 64, beams=3)[0] != steps
    assert all(1 <= r <= s <= m for r, s, m in zip(RETURNED, SELECTIONS, LIMITS))
