"""``vivit_amd.utils.solve_queue.SolveQueue`` on the GPU: a flush runs on the stream its items were queued on, whichever
stream is current at the flush, and its results can be read from the stream that flushed.  4 x 4 fp32 tensors and plain
torch ops inside ``solve``; no project kernels."""
import pytest
import torch

from vivit_amd.utils.solve_queue import SolveQueue

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]
DEV = torch.device("cuda:0")


def recording_queue():
    calls = []

    def solve(items):
        out = torch.stack(items) * 2.0 + 1.0
        calls.append((torch.cuda.current_stream(DEV), len(items), out))
        return [out]

    return SolveQueue(solve), calls


def queue_three(queue):
    """Three matrices made and queued on the current stream: full of 0, 1 and 2."""
    for i in range(3):
        queue.add(torch.full((4, 4), float(i), device=DEV), (4,), torch.full((4, 4), float(i), device=DEV))


EXPECTED = (torch.arange(3.0) * 2.0 + 1.0).view(3, 1, 1).expand(3, 4, 4)


@pytest.mark.parametrize("flush_on_the_queue_stream", [False, True], ids=["foreign", "same"])
def test_flush_runs_on_the_stream_of_the_adds(flush_on_the_queue_stream):
    queue, calls = recording_queue()
    s1 = torch.cuda.Stream(DEV)
    default = torch.cuda.current_stream(DEV)
    assert default != s1
    with torch.cuda.stream(s1):
        queue_three(queue)
        assert [key[-1] for key in queue.pending] == [s1] and [key[:-1] for key in queue.pending] == [(DEV, 4)]
        if flush_on_the_queue_stream:
            queue.flush_all()
            out_host = calls[0][2].cpu()
    if not flush_on_the_queue_stream:
        assert torch.cuda.current_stream(DEV) == default
        queue.flush_all()
        out_host = calls[0][2].cpu()                       # read from the default stream, which the flush made wait for s1
    assert not queue.pending and len(calls) == 1
    stream, count, _ = calls[0]
    assert stream == s1 and count == 3
    assert torch.equal(out_host, EXPECTED)
    assert torch.cuda.current_stream(DEV) == default       # the flush left the current stream as it found it


def test_one_size_on_two_streams_is_two_keys_and_two_solves():
    queue, calls = recording_queue()
    s1 = torch.cuda.Stream(DEV)
    default = torch.cuda.current_stream(DEV)
    with torch.cuda.stream(s1):
        queue_three(queue)
    queue_three(queue)
    assert [key[-1] for key in queue.pending] == [s1, default]
    assert [len(v) for v in queue.pending.values()] == [3, 3]
    queue.flush_all()
    assert [(stream, count) for stream, count, _ in calls] == [(s1, 3), (default, 3)]
    assert all(torch.equal(out.cpu(), EXPECTED) for _, _, out in calls)
