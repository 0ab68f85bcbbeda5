"""``EighComputation(batched_solve=True)``: the queue of the group hook, on the CPU.

The oracle stands in for the kernels (the launcher seam of tests/helpers.py); its ``symeig_reduce_batched`` is a loop over
the oracle's ``symeig_reduce`` that records the size of every call.  What is checked is the host logic alone: WHEN the
queue is flushed (eight matrices of one size; the remainder on the first ``get_result``), that the results are those of
``batched_solve=False`` (the reference's per-group solve, vivit/linalg/eigh.py:239-275), that the save-fields are gone
after the hook either way, and that parameter-side and data-parallel groups keep the immediate solve."""
import pytest
import torch

import vivit_amd
from helpers import FakeModule, OracleBackend, set_kernel_backend, top_k_criterion
from vivit_amd.backend.extensions import _materialised_closures


class CountingBackend(OracleBackend):
    def __init__(self):
        self.batched_calls = []
        self.single_calls = 0

    def symeig_reduce(self, G, overwrite=False):
        self.single_calls += 1
        return super().symeig_reduce(G, overwrite=overwrite)

    def symeig_reduce_batched(self, mats, overwrite=False, info_out=None):
        from vivit_amd.kernels import SymeigBatchPlan

        mats = list(mats)
        self.batched_calls.append(len(mats))
        plans = [OracleBackend.symeig_reduce(self, G) for G in mats]
        return SymeigBatchPlan(torch.stack([p.evals for p in plans]), mats[0].shape[0], plans)


@pytest.fixture
def backend():
    b = CountingBackend()
    set_kernel_backend(b)
    yield b
    set_kernel_backend(None)


def factors(count, C, N, shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(C, N, *shape, generator=g) / N ** 0.5 for _ in range(count)]


def run(V, N_total, subsampling=None, k=3, **kwargs):
    comp = vivit_amd.EighComputation(subsampling=subsampling, warn_small_eigvals=0.0, **kwargs)
    params = [torch.nn.Parameter(torch.zeros(*v.shape[2:])) for v in V]
    for p, v in zip(params, V):
        setattr(p, comp._savefield, _materialised_closures(v))
    groups = [{"params": [p], "criterion": top_k_criterion(k)} for p in params]
    comp.get_extension_hook(groups)(FakeModule(params, N_total))
    assert all(not hasattr(p, comp._savefield) for p in params), "save-fields are deleted in the hook, queued or not"
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
    assert got[17][0] is first[0]

    plain, plain_groups = run(V, 5 if subsampling is None else 20, subsampling=subsampling)
    assert backend.batched_calls == [8, 8, 3] and backend.single_calls == 19   # the default never queues
    for (wa, ea), g in zip(got, plain_groups):
        wb, eb = plain.get_result(g)
        assert wa.shape == (3,) and torch.equal(wa, wb)
        assert len(ea) == len(eb) == 1 and ea[0].shape == (3, 7) and torch.equal(ea[0], eb[0])


def test_sizes_are_queued_apart(backend):
    V = factors(9, 2, 5, (7,)) + factors(9, 3, 5, (7,), seed=1)     # n = 10 and n = 15, nine of each
    order = [0, 9, 1, 10, 2, 11, 3, 12, 4, 13, 5, 14, 6, 15, 7, 16, 8, 17]
    V = [V[i] for i in order]
    comp, groups = run(V, 5, batched_solve=True)
    assert backend.batched_calls == [8, 8]
    shapes = [tuple(comp.get_result(g)[1][0].shape) for g in groups]
    assert sorted(backend.batched_calls) == [1, 1, 8, 8]
    assert shapes == [(3, 7)] * 18


def test_multi_parameter_group_is_queued_with_all_its_closures(backend):
    V = factors(3, 2, 5, (7,)) + factors(1, 2, 5, (4, 3), seed=2)
    comp = vivit_amd.EighComputation(warn_small_eigvals=0.0, batched_solve=True)
    plain = vivit_amd.EighComputation(warn_small_eigvals=0.0)
    results = []
    for c in (comp, plain):
        params = [torch.nn.Parameter(torch.zeros(*v.shape[2:])) for v in V]
        for p, v in zip(params, V):
            setattr(p, c._savefield, _materialised_closures(v))
        group = {"params": params, "criterion": top_k_criterion(4)}
        c.get_extension_hook([group])(FakeModule(params, 5))
        assert all(not hasattr(p, c._savefield) for p in params)
        results.append(c.get_result(group))
    assert backend.batched_calls == [1] and backend.single_calls == 1
    (wa, ea), (wb, eb) = results
    assert torch.equal(wa, wb) and [e.shape for e in ea] == [(4, 7)] * 3 + [(4, 4, 3)]
    assert all(torch.equal(a, b) for a, b in zip(ea, eb))


def test_unknown_group_raises_key_error(backend):
    comp, groups = run(factors(3, 2, 5, (7,)), 5, batched_solve=True)
    with pytest.raises(KeyError):
        comp.get_result({"params": [], "criterion": None})
    assert backend.batched_calls == [3]          # (the look-up flushed what was waiting)
    assert comp.get_result(groups[0])[0].shape == (3,)


def test_parameter_side_groups_are_solved_at_once(backend):
    """``side='auto'`` with fewer parameters than Gram rows: the group is solved on its parameter side in the hook."""
    V = factors(3, 2, 5, (3,))     # P = 3 < n = 10
    comp, groups = run(V, 5, batched_solve=True, side="auto")
    assert backend.batched_calls == [] and not comp._pending
    assert comp.get_result(groups[0])[0].shape == (3,)
    assert backend.batched_calls == []


def test_data_parallel_keeps_the_immediate_solve():
    comp = vivit_amd.EighComputation(batched_solve=True, data_parallel=True)
    assert comp._batched_solve is False
    assert vivit_amd.EighComputation(batched_solve=True)._batched_solve is True
    assert vivit_amd.EighComputation()._batched_solve is False
