"""``DirectionalDerivativesComputation`` / ``DirectionalDampedNewtonComputation`` with ``batched_solve=True``: the queue of
the group hook, on the CPU.

The oracle stands in for the kernels (the launcher seam of tests/helpers.py).  Its ``symeig_reduce_batched`` is a loop over
the oracle's ``symeig_reduce`` that records the size of every call, its ``gram_directions_batched`` composes the oracle's own
``gemm_tn`` + ``scale_cols_rsqrt_`` + ``gemm_nn`` + ``dir_curvature`` -- the four launches of the immediate mode -- so both
modes compute the same numbers in the same order and are compared with ``torch.equal``.  What is checked is the host logic
alone: WHEN a queue is flushed (eight groups under one key; the remainder on the first ``get_result``), that gammas, lambdas
and Newton steps are those of ``batched_solve=False`` (vivit/optim/directional_damped_newton.py:304-373 per group), that
the save-fields are gone after the hook either way, and that data-parallel computations keep the immediate solve."""
import pytest
import torch

import vivit_amd
from helpers import FakeModule, OracleBackend, set_kernel_backend, top_k_criterion
from vivit_amd.backend.extensions import LinearFactor


class CountingBackend(OracleBackend):
    def __init__(self):
        self.batched_calls = []       # sizes of the symeig_reduce_batched calls
        self.direction_calls = []     # sizes of the gram_directions_batched calls
        self.single_calls = 0

    def symeig_reduce(self, G, overwrite=False):
        self.single_calls += 1
        return super().symeig_reduce(G, overwrite=overwrite)

    def symeig_reduce_batched(self, mats, overwrite=False, info_out=None):
        from vivit_amd.kernels import SymeigBatchPlan

        mats = list(mats)
        assert not overwrite, "the Gram matrices are read again by the directions kernel"
        self.batched_calls.append(len(mats))
        plans = [OracleBackend.symeig_reduce(self, G) for G in mats]
        return SymeigBatchPlan(torch.stack([p.evals for p in plans]), mats[0].shape[0], plans)

    def gram_directions_batched(self, grams, Zts, evals, VtGs, C, N, alpha_gram, alpha_gamma, lambda_scale):
        assert len(grams) == len(Zts) == len(evals) == len(VtGs)
        self.direction_calls.append(len(grams))
        gammas, lambdas = [], []
        for G, Zt, w, VtG in zip(grams, Zts, evals, VtGs):
            assert Zt.shape == (w.numel(), C * N) and G.shape == (C * N, C * N) and VtG.shape[0] == C * N
            E = Zt.T.contiguous()
            gam = self.gemm_tn(VtG, E, alpha=alpha_gamma)
            self.scale_cols_rsqrt_(gam, w)
            GE = self.gemm_nn(G, E, alpha=alpha_gram)
            gammas.append(gam)
            lambdas.append(self.dir_curvature(GE, w, C, N, scale=lambda_scale))
        return gammas, lambdas


@pytest.fixture
def backend():
    b = CountingBackend()
    set_kernel_backend(b)
    yield b
    set_kernel_backend(None)


def factors(count, C, N, shape, N_grad=None, seed=0):
    g = torch.Generator().manual_seed(seed)
    V = [torch.randn(C, N, *shape, generator=g) / N ** 0.5 for _ in range(count)]
    G = [torch.randn(N if N_grad is None else N_grad, *shape, generator=g) / N for _ in range(count)]
    return V, G


def recording_damping(log):
    """A ``damping`` callback that records what it was called with; the damping depends on all four arguments, so a
    group that was handed another group's tensors ends with another step."""

    def damping(evals, evecs, gammas, lambdas):
        log.append((evals, evecs, gammas, lambdas))
        return 1.0 + 0.1 * evals + evecs.abs().sum(0) + gammas.abs().mean(0) + lambdas.mean(0)

    return damping


def attach(params, V, G, comp):
    for p, v, g in zip(params, V, G):
        setattr(p, comp._savefield_ggn, v if isinstance(v, LinearFactor) else v.clone())
        setattr(p, comp._savefield_grad, g if isinstance(g, LinearFactor) else g.clone())


def run(cls, V, G, N_total, k=3, logs=None, **kwargs):
    """One group per factor through ``cls``; returns ``(computation, groups)`` after the pass (nothing looked up yet)."""
    comp = cls(warn_small_eigvals=0.0, **kwargs)
    params = [torch.nn.Parameter(torch.zeros(*v.shape[2:])) for v in V]
    attach(params, V, G, comp)
    groups = []
    for i, p in enumerate(params):
        group = {"params": [p], "criterion": top_k_criterion(k)}
        if cls is vivit_amd.DirectionalDampedNewtonComputation:
            group["damping"] = recording_damping(logs[i] if logs is not None else [])
        groups.append(group)
    comp.get_extension_hook(groups)(FakeModule(params, N_total))
    assert all(not hasattr(p, comp._savefield_ggn) and not hasattr(p, comp._savefield_grad) for p in params), \
        "save-fields are deleted in the hook, queued or not"
    return comp, groups


SUBSAMPLINGS = [
    pytest.param({}, 5, 5, id="full"),
    pytest.param({"subsampling_ggn": [0, 1, 2, 3, 4], "subsampling_grad": [0, 2, 4, 6, 8, 10, 12]}, 5, 7, id="subsampled"),
]


@pytest.mark.parametrize("kwargs, N, N_grad", SUBSAMPLINGS)
def test_nineteen_groups_directional_derivatives(backend, kwargs, N, N_grad):
    cls = vivit_amd.DirectionalDerivativesComputation
    N_total = 5 if not kwargs else 20
    V, G = factors(19, 2, N, (7,), N_grad=N_grad)
    comp, groups = run(cls, V, G, N_total, batched_solve=True, **kwargs)
    assert backend.batched_calls == [8, 8] and backend.direction_calls == [8, 8] and backend.single_calls == 0
    first = comp.get_result(groups[17])                    # the other three on the first get_result
    assert backend.batched_calls == [8, 8, 3] and backend.direction_calls == [8, 8, 3]
    got = [comp.get_result(g) for g in groups]
    assert backend.batched_calls == [8, 8, 3] and backend.single_calls == 0
    assert got[17][0] is first[0]

    plain, plain_groups = run(cls, V, G, N_total, **kwargs)
    assert backend.batched_calls == [8, 8, 3] and backend.single_calls == 19   # the default never queues
    for (ga, la), g in zip(got, plain_groups):
        gb, lb = plain.get_result(g)
        assert ga.shape == (N_grad, 3) and la.shape == (N, 3)
        assert torch.equal(ga, gb) and torch.equal(la, lb)


@pytest.mark.parametrize("kwargs, N, N_grad", SUBSAMPLINGS)
def test_nineteen_groups_newton_steps_and_callbacks(backend, kwargs, N, N_grad):
    cls = vivit_amd.DirectionalDampedNewtonComputation
    N_total = 5 if not kwargs else 20
    V, G = factors(19, 2, N, (7,), N_grad=N_grad)
    logs = [[] for _ in V]
    comp, groups = run(cls, V, G, N_total, logs=logs, batched_solve=True, **kwargs)
    assert backend.batched_calls == [8, 8] and backend.direction_calls == [8, 8] and backend.single_calls == 0
    assert [len(log) for log in logs] == [1] * 16 + [0] * 3      # the flushed groups went on to their damping callback
    got = [comp.get_result(g) for g in groups]
    assert backend.batched_calls == [8, 8, 3] and backend.direction_calls == [8, 8, 3] and backend.single_calls == 0
    assert [len(log) for log in logs] == [1] * 19                # every group's callback exactly once

    plain_logs = [[] for _ in V]
    plain, plain_groups = run(cls, V, G, N_total, logs=plain_logs, **kwargs)
    assert backend.single_calls == 19
    for sa, g in zip(got, plain_groups):
        sb = plain.get_result(g)
        assert len(sa) == len(sb) == 1 and sa[0].shape == (7,) and torch.equal(sa[0], sb[0])
    # each callback saw ITS group's (evals [K], evecs [n, K], gammas [N_grad, K], lambdas [N, K])
    for (log,), (plain_log,) in zip(logs, plain_logs):
        assert [tuple(t.shape) for t in log] == [(3,), (2 * N, 3), (N_grad, 3), (N, 3)]
        assert all(torch.equal(a, b) for a, b in zip(log, plain_log))
    assert len({log[0][0].sum().item() for log in logs}) == 19   # (the groups do differ)


def test_two_sizes_interleaved_are_queued_apart(backend):
    cls = vivit_amd.DirectionalDampedNewtonComputation
    Va, Ga = factors(9, 2, 5, (7,))
    Vb, Gb = factors(9, 3, 5, (7,), seed=1)               # n = 10 and n = 15, nine of each
    order = [0, 9, 1, 10, 2, 11, 3, 12, 4, 13, 5, 14, 6, 15, 7, 16, 8, 17]
    V, G = [(Va + Vb)[i] for i in order], [(Ga + Gb)[i] for i in order]
    comp, groups = run(cls, V, G, 5, batched_solve=True)
    assert backend.batched_calls == [8, 8] and backend.direction_calls == [8, 8]
    assert sorted(len(items) for items in comp._queue.pending.values()) == [1, 1]
    assert sorted(key[1:4] for key in comp._queue.pending) == [(10, 2, 5), (15, 3, 5)]     # (device, n, C, M, stream)
    got = [comp.get_result(g) for g in groups]
    assert sorted(backend.batched_calls) == [1, 1, 8, 8] and sorted(backend.direction_calls) == [1, 1, 8, 8]
    plain, plain_groups = run(cls, V, G, 5)
    for sa, g in zip(got, plain_groups):
        assert torch.equal(sa[0], plain.get_result(g)[0])


def test_another_gradient_subsample_is_another_queue(backend):
    """M (the number of per-sample gradients) is part of the key: the kernel has one M per call."""
    cls = vivit_amd.DirectionalDerivativesComputation
    comp = cls(warn_small_eigvals=0.0, batched_solve=True)
    comp._queue.add({"V_t_V": torch.eye(10).view(2, 5, 2, 5), "V_t_g_n": torch.ones(2, 5, 5)}, {"criterion": top_k_criterion(1)}, 5)
    comp._queue.add({"V_t_V": torch.eye(10).view(2, 5, 2, 5), "V_t_g_n": torch.ones(2, 5, 3)}, {"criterion": top_k_criterion(1)}, 5)
    assert sorted(key[1:4] for key in comp._queue.pending) == [(10, 2, 3), (10, 2, 5)]


@pytest.mark.parametrize("cls", [vivit_amd.DirectionalDerivativesComputation, vivit_amd.DirectionalDampedNewtonComputation])
def test_multi_parameter_group_factorised_and_dense(backend, cls):
    """A group of one factorised Linear weight and one dense parameter is queued whole: its Gram matrix and ``V_t_g_n`` are
    the sums over both, the Newton step is back-projected through both kinds of factor."""
    C, N, O, I = 2, 5, 4, 3
    g = torch.Generator().manual_seed(3)
    s, z = torch.randn(C, N, O, generator=g) / N ** 0.5, torch.randn(N, I, generator=g)
    delta = torch.randn(N, O, generator=g) / N
    Vb, gb = torch.randn(C, N, O, generator=g) / N ** 0.5, torch.randn(N, O, generator=g) / N
    results = []
    for batched in (True, False):
        comp = cls(warn_small_eigvals=0.0, factorised=True, batched_solve=batched)
        params = [torch.nn.Parameter(torch.zeros(O, I)), torch.nn.Parameter(torch.zeros(O))]
        attach(params, [LinearFactor(s, z), Vb], [LinearFactor(delta, z), gb], comp)
        group = {"params": params, "criterion": top_k_criterion(4), "damping": recording_damping([])}
        comp.get_extension_hook([group])(FakeModule(params, N))
        assert all(not hasattr(p, comp._savefield_ggn) and not hasattr(p, comp._savefield_grad) for p in params)
        assert sum(len(items) for items in comp._queue.pending.values()) == (1 if batched else 0)
        results.append(comp.get_result(group))
        assert not comp._queue.pending
    assert backend.batched_calls == [1] and backend.direction_calls == [1] and backend.single_calls == 1
    a, b = results
    assert len(a) == len(b) == 2 and all(torch.equal(x, y) for x, y in zip(a, b))
    if cls is vivit_amd.DirectionalDampedNewtonComputation:
        assert [tuple(t.shape) for t in a] == [(O, I), (O,)]


@pytest.mark.parametrize("cls", [vivit_amd.DirectionalDerivativesComputation, vivit_amd.DirectionalDampedNewtonComputation])
def test_unknown_group_raises_key_error_after_flushing(backend, cls):
    V, G = factors(3, 2, 5, (7,))
    comp, groups = run(cls, V, G, 5, batched_solve=True)
    assert backend.batched_calls == []
    with pytest.raises(KeyError):
        comp.get_result({"params": [], "criterion": None})
    assert backend.batched_calls == [3] and backend.direction_calls == [3]   # (the look-up flushed what was waiting)
    assert len(comp.get_result(groups[0])) in (1, 2)
    assert backend.batched_calls == [3]


@pytest.mark.parametrize("cls", [vivit_amd.DirectionalDerivativesComputation, vivit_amd.DirectionalDampedNewtonComputation])
def test_data_parallel_keeps_the_immediate_solve(cls):
    assert cls(batched_solve=True, data_parallel=True)._batched_solve is False
    assert cls(batched_solve=True)._batched_solve is True
    assert cls()._batched_solve is False


def test_optimizer_forwards_batched_solve(backend):
    from vivit_amd.optim import DirectionalDampedNewton

    seen = {}

    class Recording(vivit_amd.DirectionalDampedNewtonComputation):
        def __init__(self, **kwargs):
            seen.update(kwargs)
            super().__init__(**kwargs)

    import vivit_amd.optim.optimizer as optimizer_module

    p = torch.nn.Parameter(torch.zeros(3))
    opt = DirectionalDampedNewton([p], criterion=top_k_criterion(1), damping=recording_damping([]), backpack=None,
                                  batched_solve=True, warn_small_eigvals=0.0)
    original = optimizer_module.DirectionalDampedNewtonComputation
    optimizer_module.DirectionalDampedNewtonComputation = Recording
    try:
        with pytest.raises(TypeError):     # backpack=None is not a context manager: the computation was built before
            opt.step(lambda: (p ** 2).sum())
    finally:
        optimizer_module.DirectionalDampedNewtonComputation = original
    assert seen == {"batched_solve": True, "warn_small_eigvals": 0.0}
