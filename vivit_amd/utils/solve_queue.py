"""The queue behind every ``batched_solve=True`` mode: problems of one size wait for a solve that takes them together."""
import contextlib
from typing import Callable, Dict, List, Tuple

import torch
from torch import Tensor

FLUSH_AT = 8  # problems of one size that make a full launch of the batched eigensolvers (one per XCD)


class SolveQueue:
    """Items wait under ``(device, *sizes, stream)``; ``solve(items) -> tensors handed out`` runs once per flush of a key.

    A key is flushed as soon as :data:`FLUSH_AT` items wait under it, the rest by :meth:`flush_all` (the computations call
    it first thing in ``get_result``), oldest key first.  The items leave the queue before ``solve`` runs, so a solve that
    raises does not leave them behind.

    Streams -- the one place where the package orders streams and deals with the caching allocator by hand.  The hooks run
    on the backend's side stream (vivit_amd/backend/engine.py), so that is where the queued tensors are allocated and
    written; ``get_result`` runs on the caller's.  ``stream`` is the stream current on the tensor's device at :meth:`add`
    (``None`` off the GPU) and EVERY flush of the key runs on it: behind all work on the queued tensors by stream order, on
    memory that belongs to that stream as far as the allocator is concerned (no ``record_stream`` for the inputs).  When a
    flush finds another stream current, that stream then waits for the queue's and every tensor that ``solve`` returned is
    recorded on it.  Nothing else synchronises."""

    def __init__(self, solve: Callable[[List], List[Tensor]]):
        self._solve = solve
        self.pending: Dict[Tuple, List] = {}

    def add(self, tensor: Tensor, sizes: Tuple[int, ...], item):
        """Queue ``item`` under the device and current stream of ``tensor`` (one of the item's operands) and ``sizes``."""
        stream = torch.cuda.current_stream(tensor.device) if tensor.is_cuda else None
        key = (tensor.device, *sizes, stream)
        self.pending.setdefault(key, []).append(item)
        if len(self.pending[key]) >= FLUSH_AT:
            self.flush(key)

    def flush_all(self):
        for key in list(self.pending):
            self.flush(key)

    def flush(self, key):
        items = self.pending.pop(key, [])
        if not items:
            return
        stream = key[-1]
        current = None if stream is None else torch.cuda.current_stream(key[0])
        foreign = stream is not None and current != stream
        with torch.cuda.stream(stream) if foreign else contextlib.nullcontext():
            results = self._solve(items)
        if foreign:
            current.wait_stream(stream)
            for t in results:
                t.record_stream(current)
