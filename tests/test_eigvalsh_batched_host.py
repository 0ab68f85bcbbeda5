"""``EigvalshComputation(batched_solve=True)``: the queue of the group hook, on the CPU.

The oracle stands in for the kernels (the launcher seam of tests/helpers.py); its ``symeigvals_batched`` is a loop over the
oracle's values-only ``symeig`` that records the size of every call.  What is checked is the host logic alone: WHEN the
queue is flushed (eight matrices of one size; the remainder on the first ``get_result``), that the results are those of
``batched_solve=False`` (the reference's per-group ``Tensor.symeig``, vivit/linalg/eigvalsh.py:221), and the
``KeyError`` of the reference for a group that never ran (vivit/linalg/eigvalsh.py:60-66)."""
import pytest
import torch

import vivit_amd
from helpers import FakeModule, OracleBackend, set_kernel_backend
from vivit_amd.backend.extensions import _materialised_closures


class CountingBackend(OracleBackend):
    def __init__(self):
        self.batched_calls = []
        self.single_calls = 0

    def symeig(self, G, eigenvectors=False, overwrite=False):
        self.single_calls += 1
        return super().symeig(G, eigenvectors=eigenvectors, overwrite=overwrite)

    def symeigvals_batched(self, mats, overwrite=False, info_out=None):
        mats = list(mats)
        self.batched_calls.append(len(mats))
        return torch.stack([OracleBackend.symeig(self, G, eigenvectors=False)[0] for G in mats])


@pytest.fixture
def backend():
    b = CountingBackend()
    set_kernel_backend(b)
    yield b
    set_kernel_backend(None)


def factors(count, C, N, shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(C, N, *shape, generator=g) / N ** 0.5 for _ in range(count)]


def run(V, N_total, subsampling=None, **kwargs):
    comp = vivit_amd.EigvalshComputation(subsampling=subsampling, **kwargs)
    params = [torch.nn.Parameter(torch.zeros(*v.shape[2:])) for v in V]
    for p, v in zip(params, V):
        setattr(p, comp._savefield, _materialised_closures(v))
    groups = [{"params": [p]} for p in params]
    comp.get_extension_hook(groups)(FakeModule(params, N_total))
    return comp, groups


@pytest.mark.parametrize("subsampling", [None, [0, 1, 2, 3, 4]])
def test_nineteen_groups_flush_eight_eight_three(backend, subsampling):
    C, N = 2, 5
    V = factors(19, C, N, (7,))
    comp, groups = run(V, 5 if subsampling is None else 20, subsampling=subsampling, batched_solve=True)
    assert backend.batched_calls == [8, 8] and backend.single_calls == 0   # two full launches during the pass
    first = comp.get_result(groups[17])                                     # ... the other three on the first get_result
    assert backend.batched_calls == [8, 8, 3]
    got = [comp.get_result(g) for g in groups]
    assert backend.batched_calls == [8, 8, 3] and backend.single_calls == 0
    assert got[17] is first

    plain, plain_groups = run(V, 5 if subsampling is None else 20, subsampling=subsampling)
    assert backend.batched_calls == [8, 8, 3] and backend.single_calls == 19   # the default never queues
    for a, g in zip(got, plain_groups):
        b = plain.get_result(g)
        assert a.shape == (C * N,) and torch.equal(a, b)


def test_sizes_are_queued_apart(backend):
    V = factors(9, 2, 5, (7,)) + factors(9, 3, 5, (7,), seed=1)     # n = 10 and n = 15, nine of each
    order = [0, 9, 1, 10, 2, 11, 3, 12, 4, 13, 5, 14, 6, 15, 7, 16, 8, 17]
    V = [V[i] for i in order]
    comp, groups = run(V, 5, batched_solve=True)
    assert backend.batched_calls == [8, 8]
    shapes = [tuple(comp.get_result(g).shape) for g in groups]
    assert sorted(backend.batched_calls) == [1, 1, 8, 8]
    assert shapes == [(10,), (15,)] * 9


def test_unknown_group_raises_key_error(backend):
    comp, groups = run(factors(3, 2, 5, (7,)), 5, batched_solve=True)
    with pytest.raises(KeyError):
        comp.get_result({"params": []})
    assert backend.batched_calls == [3]          # (the look-up flushed what was waiting)
    assert comp.get_result(groups[0]).shape == (10,)
    fresh = vivit_amd.EigvalshComputation(batched_solve=True)
    with pytest.raises(KeyError):
        fresh.get_result(groups[0])


def test_parameter_side_groups_are_solved_at_once(backend):
    """``side='auto'`` with fewer parameters than Gram rows: the group is solved on its parameter side in the hook."""
    V = factors(3, 2, 5, (3,))     # P = 3 < n = 10
    comp, groups = run(V, 5, batched_solve=True, side="auto")
    assert backend.batched_calls == [] and not comp._pending
    assert comp.get_result(groups[0]).shape == (10,)
    assert backend.batched_calls == []
