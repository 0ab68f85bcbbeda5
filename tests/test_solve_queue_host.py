"""``vivit_amd.utils.solve_queue.SolveQueue`` on the CPU, driven directly: WHEN a key is flushed, with WHAT, in which
order, and what a raising ``solve`` leaves behind.  No kernels; ``solve`` only records its calls."""
import pytest
import torch

from vivit_amd.utils.solve_queue import FLUSH_AT, SolveQueue


def recording_queue():
    calls = []

    def solve(items):
        calls.append(list(items))
        return [torch.zeros(1)]

    return SolveQueue(solve), calls


def test_eight_adds_make_one_solve_in_insertion_order():
    assert FLUSH_AT == 8
    queue, calls = recording_queue()
    t = torch.zeros(4, 4)
    for i in range(7):
        queue.add(t, (4,), i)
    assert calls == [] and [len(v) for v in queue.pending.values()] == [7]
    queue.add(t, (4,), 7)
    assert calls == [list(range(8))] and not queue.pending
    queue.add(t, (4,), 8)                                  # the ninth waits
    assert calls == [list(range(8))] and list(queue.pending.values()) == [[8]]
    assert list(queue.pending) == [(t.device, 4, None)]


def test_two_size_tuples_interleaved_are_queued_apart():
    queue, calls = recording_queue()
    t = torch.zeros(4, 4)
    for i in range(9):
        queue.add(t, (15, 3, 5), ("b", i))                 # this key is created first ...
        queue.add(t, (10, 2, 5), ("a", i))
    assert calls == [[("b", i) for i in range(8)], [("a", i) for i in range(8)]]   # one full solve per key during the adds
    # ... and is re-created first after its flush: the remainders leave in the order the keys were created
    assert list(queue.pending) == [(t.device, 15, 3, 5, None), (t.device, 10, 2, 5, None)]
    assert all(key[-1] is None for key in queue.pending), "CPU tensors have no stream"
    queue.flush_all()
    assert calls[2:] == [[("b", 8)], [("a", 8)]] and not queue.pending
    queue.flush_all()
    assert len(calls) == 4


def test_a_raising_solve_leaves_nothing_queued_under_its_key():
    seen = []

    def solve(items):
        seen.append(list(items))
        if "bad" in items:
            raise RuntimeError("solve failed")
        return []

    queue = SolveQueue(solve)
    t = torch.zeros(4, 4)
    queue.add(t, (4,), "bad")
    queue.add(t, (5,), "good")
    bad_key, good_key = list(queue.pending)
    with pytest.raises(RuntimeError, match="solve failed"):
        queue.flush(bad_key)
    assert seen == [["bad"]]
    assert bad_key not in queue.pending and queue.pending == {good_key: ["good"]}   # the other key is untouched
    queue.flush_all()
    assert seen == [["bad"], ["good"]] and not queue.pending


def test_a_raising_solve_propagates_from_the_eighth_add_and_from_flush_all():
    def solve(items):
        raise RuntimeError("solve failed")

    queue = SolveQueue(solve)
    t = torch.zeros(4, 4)
    for i in range(7):
        queue.add(t, (4,), i)
    with pytest.raises(RuntimeError):
        queue.add(t, (4,), 7)
    assert not queue.pending
    queue.add(t, (4,), 8)
    with pytest.raises(RuntimeError):
        queue.flush_all()
    assert not queue.pending


def test_flush_of_an_unknown_or_empty_key_is_a_no_op():
    queue, calls = recording_queue()
    queue.flush((torch.device("cpu"), 4, None))            # never queued
    queue.pending[(torch.device("cpu"), 5, None)] = []     # queued and empty
    queue.flush((torch.device("cpu"), 5, None))
    queue.flush_all()
    assert calls == []
