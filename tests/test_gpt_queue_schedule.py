"""CPU: the host model of the sentence queue's scheduling policy (mi355tts.indextts.queue_schedule; the policy is stated in
include/mi355tts.h, "sentence queue").  The GPU tests hold mi_gpt_generate_queue's stats against this model; here the model
itself is held against hand-checked cases and against properties every schedule must have."""
import math

import numpy as np
import pytest

from mi355tts.indextts import lockstep_steps, queue_schedule


def test_refill_beats_lockstep_groups():
    lens = [65, 17, 17, 17, 17]
    steps, passes = queue_schedule([10] * 5, lens, lens, 2, 96)
    assert steps == 64
    assert passes == [[(0, 0), (1, 1)], [(2, 1)], [(3, 1)], [(4, 1)]]
    assert lockstep_steps(lens, 2) == 96


def test_early_stops_and_retire_after_the_prompt_pass():
    steps, passes = queue_schedule([10] * 6, [40] * 6, [40, 3, 1, 25, 40, 9], 3, 96)
    assert steps == 55
    # sentence 2 (one token: its token 0 is a stop id) retires after its prompt pass: sentence 3 follows with no step between
    assert passes == [[(0, 0), (1, 1), (2, 2)], [(3, 2)], [(4, 1)], [(5, 2)]]


def test_scratch_capacity_splits_a_pass():
    steps, passes = queue_schedule([60, 50, 10, 5], [4] * 4, [4] * 4, 4, 96)
    assert passes == [[(0, 0)], [(1, 1), (2, 2), (3, 3)]]
    assert steps == 3


def test_zero_limit_takes_no_slot():
    steps, passes = queue_schedule([5, 5, 5], [3, 0, 3], [3, 0, 3], 2, 64)
    assert passes == [[(0, 0), (2, 1)]] and steps == 2
    assert queue_schedule([5], [0], [0], 4, 64) == (0, [])


def test_rejects_inconsistent_arguments():
    with pytest.raises(ValueError):
        queue_schedule([5, 5], [3], [3], 2, 64)
    with pytest.raises(ValueError):
        queue_schedule([5], [3], [4], 2, 64)          # produced more than the limit
    with pytest.raises(ValueError):
        queue_schedule([5], [3], [0], 2, 64)          # a sentence with a limit produces at least its token 0


@pytest.mark.parametrize("seed", range(12))
def test_schedule_properties(seed):
    """Even seeds: no early stop (lengths == max_new); odd seeds: every sentence stops somewhere up to its limit.

    The bound against lock-step groups.  Both schedules start sentences in index order on `slots` identical slots and a prompt
    pass costs no step, so by induction over the sentences no sentence starts later in the queue than in the lock-step
    schedule, PROVIDED a sentence holds its slot no longer in the queue than there.  Without early stops it holds it for
    exactly length - 1 steps (every run of steps ends at the nearest limit), lock-step for at least that: steps <= lock-step.
    With early stops the queue sees a stop only at the end of a run of up to 16 steps, so it may hold the slot for up to
    length - 1 + 15 steps and the plain bound is false: limits [10, 59, 32, 18, 21, 31, 1, 46, 2, 68] with lengths
    [4, 22, 29, 5, 1, 21, 1, 23, 1, 49] in 12 slots take 63 steps against lock-step's 48, whose 16-step runs happen to end on
    the longest sentence's last token.  What the induction gives there is the lock-step count of sentences 15 tokens longer."""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(1, 40))
    slots = int(rng.integers(1, 17))
    max_seq = int(rng.integers(64, 400))
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
        assert p and len({s for _, s in p}) == len(p)                             # one sentence per slot in a pass
        assert all(0 <= s < min(slots, n) for _, s in p)
        assert len(p) == 1 or sum(rows[i] for i, _ in p) <= max_seq               # the scratch bound (a lone sentence always fits)
    # a slot is reused only by a later sentence (that its earlier owner is done by then: the test below)
    last_in_slot = {}
    for p in passes:
        for i, s in p:
            assert s not in last_in_slot or last_in_slot[s] < i
            last_in_slot[s] = i
    longest = max(lens) if lens else 0
    assert steps >= math.ceil(max(longest - 1, 0))
    if seed % 2 == 0:
        assert steps <= lockstep_steps(lens, slots)
    else:
        assert steps <= lockstep_steps([x + 15 if x else 0 for x in lens], slots)


def test_early_stops_can_cost_more_steps_than_lockstep():
    """The counter-example of the docstring above, pinned: the plain bound is a property of sentences that run to their limits."""
    limit = [10, 59, 32, 18, 21, 31, 1, 46, 2, 68]
    lens = [4, 22, 29, 5, 1, 21, 1, 23, 1, 49]
    steps, passes = queue_schedule([8] * 10, limit, lens, 12, 1024)
    assert len(passes) == 1 and steps == 63 and lockstep_steps(lens, 12) == 48
    assert steps <= lockstep_steps([x + 15 for x in lens], 12)
    assert queue_schedule([8] * 10, lens, lens, 12, 1024)[0] == 48


def test_no_slot_holds_two_live_sentences():
    """Simulate the decode against the passes the model returns: when a sentence enters a slot, the one before it there is done."""
    rng = np.random.default_rng(7)
    for _ in range(20):
        n, slots = int(rng.integers(2, 30)), int(rng.integers(1, 9))
        limit = rng.integers(1, 50, n).tolist()
        lens = [int(rng.integers(1, m + 1)) for m in limit]
        rows = [8] * n
        steps, passes = queue_schedule(rows, limit, lens, slots, 64)
        # re-run the policy's clock with the model's passes as the only source of admissions
        owner, got, pi, total = {}, [0] * n, 0, 0
        while True:
            while pi < len(passes) and all(s not in owner for _, s in passes[pi]):
                for i, s in passes[pi]:
                    owner[s] = i
                    got[i] = 1
                pi += 1
            for s in [s for s, i in owner.items() if got[i] >= lens[i]]:
                del owner[s]
            if pi < len(passes) and all(s not in owner for _, s in passes[pi]):
                continue
            if not owner:
                break
            c = min(16, min(limit[i] - got[i] for i in owner.values()))
            assert c >= 1
            total += c
            for i in owner.values():
                got[i] = min(lens[i], got[i] + c)
        assert pi == len(passes) and total == steps and got == lens
