"""``DirectionalDerivativesComputation`` / ``DirectionalDampedNewtonComputation`` with ``batched_solve=True`` on the GPU:
the queue of tests/test_optim_batched_host.py feeding the real kernels (``symeig_reduce_batched``, the batched select and
``gram_directions_batched``).

(a) the golden cases ``multikernel`` (n = 320: a batch of one through the batched kernels) and ``mlp_small`` (n = 12: the
    looping route) against the reference's recorded outputs, at exactly the tolerances of
    tests/test_api_golden.py::test_directional_derivatives_and_newton;
(b) twelve single-parameter groups with n = 1280 from ``helpers.planted_factors`` (kept directions well separated), batched
    and immediate, both against the oracle in fp64 on the same factors at the tolerances of (a); gammas in absolute value
    (the two modes use different back-transformation kernels, an eigenvector's sign is free), lambdas and steps directly;
(c) one real backward pass through an MLP of equal Linear layers with ``factorised=True`` and one group per parameter."""
import numpy as np
import pytest
import torch
from torch import nn

import vivit_amd
from helpers import FakeModule, constant_damping, golden_factors, load_golden, planted_factors, set_kernel_backend, top_k_criterion
from oracle import vivit_oracle as oracle
from vivit_amd.backend import backpack, extend

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
DEV = torch.device("cuda:0")
DD, DN = vivit_amd.DirectionalDerivativesComputation, vivit_amd.DirectionalDampedNewtonComputation


@pytest.fixture(autouse=True)
def hip_kernels():
    set_kernel_backend(None)


def close(a, b, rtol, atol):
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else b
    np.testing.assert_allclose(a.detach().cpu().numpy(), b, rtol=rtol, atol=atol)


def check_directions(gam, lam, ref_gam, ref_lam):
    """Tolerances of tests/test_api_golden.py::test_directional_derivatives_and_newton."""
    close(gam.abs(), np.abs(ref_gam), rtol=1e-4, atol=1e-4 * np.abs(ref_gam).max())
    close(lam, ref_lam, rtol=1e-4, atol=1e-5 * np.abs(ref_lam).max())


def check_steps(steps, refs):
    assert len(steps) == len(refs)
    for s, ref in zip(steps, refs):
        assert tuple(s.shape) == tuple(ref.shape)
        close(s, ref, rtol=1e-4, atol=1e-5 * max(np.abs(ref).max(), 1e-3))


def attach(params, V, G, comp):
    for p, v, g in zip(params, V, G):
        setattr(p, comp._savefield_ggn, v.clone())
        setattr(p, comp._savefield_grad, g.clone())


def waiting(comp):
    return sum(len(items) for items in comp._queue.pending.values())


@pytest.mark.parametrize("case", ["multikernel", "mlp_small"])
def test_golden_cases_through_the_queue(case):
    g = load_golden(case)
    V, G = golden_factors(g, DEV)
    N, N_total, N_grad = int(g["N"]), int(g["N_total"]), int(g["N_grad"])
    assert V[0].shape[0] * N == {"multikernel": 320, "mlp_small": 12}[case]
    sub = None if N == N_total else list(range(N))
    sub_grad = None if N_grad == N_total else list(range(N_grad))
    crit = top_k_criterion(int(g["k"]))

    comp = DD(subsampling_grad=sub_grad, subsampling_ggn=sub, warn_small_eigvals=0.0, batched_solve=True)
    params = [nn.Parameter(torch.zeros(*v.shape[2:], device=DEV)) for v in V]
    attach(params, V, G, comp)
    groups = [{"params": params, "criterion": crit}]
    comp.get_extension_hook(groups)(FakeModule(params, N_total))
    assert waiting(comp) == 1 and not comp._gammas, "the group waits in the queue"
    assert all(not hasattr(p, comp._savefield_ggn) and not hasattr(p, "grad_batch") for p in params)
    gam, lam = comp.get_result(groups[0])
    assert waiting(comp) == 0
    check_directions(gam, lam, g["gammas"], g["lambdas"])

    comp = DN(subsampling_grad=sub_grad, subsampling_ggn=sub, warn_small_eigvals=0.0, batched_solve=True)
    params = [nn.Parameter(torch.zeros(*v.shape[2:], device=DEV)) for v in V]
    attach(params, V, G, comp)
    groups = [{"params": params, "criterion": crit, "damping": constant_damping(1.0)}]
    comp.get_extension_hook(groups)(FakeModule(params, N_total))
    assert waiting(comp) == 1 and not comp._newton_steps, "the group waits in the queue"
    assert all(not hasattr(p, comp._savefield_ggn) and not hasattr(p, "grad_batch") for p in params)
    check_steps(comp.get_result(groups[0]), [g[f"newton{i}"] for i in range(len(V))])


TWELVE = dict(C=10, N=128, shape=(256,), k=10)


def twelve_groups():
    """Factors of twelve layers (n = 1280 each) and the fp64 oracle's gammas, lambdas and Newton steps on them."""
    C, N, shape, k = TWELVE["C"], TWELVE["N"], TWELVE["shape"], TWELVE["k"]
    crit, damp = top_k_criterion(k), constant_damping(1.0)
    Vs, Gs, refs = [], [], []
    for i in range(12):
        V, G = planted_factors(100 + i, C, N, [shape])
        gam, lam = oracle.directional_derivatives_group([V[0].double()], [G[0].double()], crit, N)
        step = oracle.damped_newton_group([V[0].double()], [G[0].double()], crit, damp, N)
        Vs.append(V[0].to(DEV)), Gs.append(G[0].to(DEV)), refs.append((gam.numpy(), lam.numpy(), step[0].numpy()))
    return Vs, Gs, refs, crit, damp


@pytest.fixture(scope="module")
def twelve():
    return twelve_groups()


@pytest.mark.parametrize("batched", [True, False], ids=["batched", "immediate"])
def test_twelve_groups_against_the_fp64_oracle(twelve, batched):
    Vs, Gs, refs, crit, damp = twelve
    N = TWELVE["N"]
    for cls in (DD, DN):
        comp = cls(warn_small_eigvals=0.0, batched_solve=batched)
        params = [nn.Parameter(torch.zeros(*TWELVE["shape"], device=DEV)) for _ in Vs]
        attach(params, Vs, Gs, comp)
        groups = [{"params": [p], "criterion": crit, "damping": damp} for p in params]
        comp.get_extension_hook(groups)(FakeModule(params, N))
        assert all(not hasattr(p, comp._savefield_ggn) and not hasattr(p, "grad_batch") for p in params)
        done = comp._gammas if cls is DD else comp._newton_steps
        if batched:
            assert len(done) == 8 and waiting(comp) == 4, "eight flushed during the pass, four wait"
            assert [key[1:4] for key in comp._queue.pending] == [(1280, 10, 128)]
        else:
            assert len(done) == 12 and waiting(comp) == 0
        for group, (ref_gam, ref_lam, ref_step) in zip(groups, refs):
            if cls is DD:
                gam, lam = comp.get_result(group)
                assert gam.shape == (N, 10) and lam.shape == (N, 10)
                check_directions(gam, lam, ref_gam, ref_lam)
            else:
                check_steps(comp.get_result(group), [ref_step])
        assert waiting(comp) == 0


def test_backward_pass_factorised_per_parameter_groups():
    """Five equal Linear layers, 16 classes, 16 samples: ten groups with n = 256 -- eight are flushed during the backward
    pass (on the extensions' stream), two on ``get_result``."""
    torch.manual_seed(0)
    layers = []
    for _ in range(4):
        layers += [nn.Linear(16, 16), nn.Sigmoid()]
    model = nn.Sequential(*layers, nn.Linear(16, 16)).to(DEV)
    X, y = torch.rand(16, 16, device=DEV), torch.randint(0, 16, (16,), device=DEV)
    m, lossf = extend(model), extend(nn.CrossEntropyLoss())
    crit, damp = top_k_criterion(3, must_exceed=1e-7), constant_damping(1.0)
    steps = {}
    for batched in (True, False):
        comp = DN(warn_small_eigvals=0.0, factorised=True, batched_solve=batched)
        groups = [{"params": [p], "criterion": crit, "damping": damp} for p in m.parameters()]
        m.zero_grad()
        loss = lossf(m(X), y)
        with backpack(*comp.get_extensions(), extension_hook=comp.get_extension_hook(groups)):
            loss.backward()
        assert len(groups) == 10
        assert waiting(comp) == (2 if batched else 0) and len(comp._newton_steps) == (8 if batched else 10)
        for p in m.parameters():
            assert not hasattr(p, comp._savefield_ggn) and not hasattr(p, comp._savefield_grad), "no save-field may be left"
        steps[batched] = [comp.get_result(group)[0] for group in groups]
        assert waiting(comp) == 0
    for p, a, b in zip(m.parameters(), steps[True], steps[False]):
        assert a.shape == p.shape
        check_steps([a], [b.cpu().numpy()])
    moved = sum(bool(b.abs().max() > 0) for b in steps[False])
    print(f"\n  {moved} of 10 groups have a non-zero step")
    assert moved >= 1
