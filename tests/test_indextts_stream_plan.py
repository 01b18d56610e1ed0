"""CPU: indextts.stream_plan, the host model of which vocoder windows are ready while a queue session decodes
(indextts.stream_synthesize runs it after every QueueSession.advance).  Properties over seeded random progress traces: counts
rising by at most 16 per round, limits including 0, 1, 2 and 3 codes, random chunk and halo."""
import random

import pytest

from mi355tts.indextts import stream_plan


def _trace(rng, n):
    """per round (count, done) of n sentences: each starts at a random round and grows by 1 .. 16 codes a round up to its limit"""
    limits = [rng.choice([0, 1, 2, 3, 4, 5, 17, 40, 90, 133]) for _ in range(n)]
    start = [rng.randrange(0, 6) for _ in range(n)]
    count = [0] * n
    rounds = []
    r = 0
    while True:
        for i in range(n):
            if r >= start[i] and count[i] < limits[i]:
                count[i] = min(limits[i], count[i] + rng.randint(1, 16))
        done = [r >= start[i] and count[i] == limits[i] for i in range(n)]
        rounds.append((list(count), done))
        if all(done):
            return limits, rounds
        r += 1


@pytest.mark.parametrize("seed", range(12))
def test_stream_plan_properties(seed):
    rng = random.Random(seed)
    n = rng.randint(1, 9)
    chunk, halo = rng.choice([1, 3, 8, 16, 32]), rng.choice([0, 1, 5, 16, 39])
    limits, rounds = _trace(rng, n)
    emitted = [0] * n
    got = [[] for _ in range(n)]
    for count, done in rounds:
        before = list(emitted)
        plan, emitted = stream_plan(emitted, count, done, chunk, halo)
        assert [p[0] for p in plan] == sorted(p[0] for p in plan)
        for i, a, b, lo, hi, last in plan:
            A = count[i] - 2
            # in order, no gap, no overlap
            assert a == (got[i][-1][1] if got[i] else 0) and a < b <= A
            # no window reads a row >= count - 2, while live or done
            assert 0 <= lo <= a and b <= hi <= A
            # head = tail = halo unless clipped by the sentence's ends
            assert a - lo == min(halo, a) and hi - b == min(halo, A - b)
            if done[i]:
                assert b == A and last
            else:
                assert b - a == chunk and b + halo <= A and not last
            got[i].append((a, b))
        # a window is emitted in the first round in which the rule allows it: afterwards nothing more is allowed
        for i in range(n):
            A, e = count[i] - 2, emitted[i]
            assert e >= before[i]
            if done[i]:
                assert e == max(A, 0) or A < 1
            else:
                assert not e + chunk + halo <= A
        # a second look at the same state emits nothing
        assert stream_plan(emitted, count, done, chunk, halo) == ([], emitted)
    for i in range(n):
        F = limits[i] - 2
        if F < 1:
            assert got[i] == []                    # fewer than three codes: nothing
        else:
            assert got[i][0][0] == 0 and got[i][-1][1] == F
            assert all(x[1] == y[0] for x, y in zip(got[i][:-1], got[i][1:]))


def test_stream_plan_example():
    # chunk 8, halo 4: 30 codes live -> A = 28: [0, 8) and [8, 16) are ready ([16, 24) needs 28 frames: 16 + 8 + 4 <= 28, ready too)
    plan, em = stream_plan([0], [30], [False], 8, 4)
    assert plan == [(0, 0, 8, 0, 12, False), (0, 8, 16, 4, 20, False), (0, 16, 24, 12, 28, False)] and em == [24]
    plan, em = stream_plan(em, [33], [True], 8, 4)
    assert plan == [(0, 24, 31, 20, 31, True)] and em == [31]
    assert stream_plan([0, 0, 0], [0, 1, 2], [True, True, True], 8, 4) == ([], [0, 0, 0])
    assert stream_plan([0], [3], [True], 8, 4) == ([(0, 0, 1, 0, 1, True)], [1])
    with pytest.raises(ValueError):
        stream_plan([0], [3], [True], 0, 4)
    with pytest.raises(ValueError):
        stream_plan([0], [3, 4], [True], 8, 4)
