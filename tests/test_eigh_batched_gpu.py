"""``EighComputation(batched_solve=True)`` on the GPU: the groups' Gram matrices go through the queue and
``kernels.symeig_reduce_batched`` instead of one two-phase solve per group hook.

Eigenvalues must EQUAL those of ``batched_solve=False`` (the batched reduction reproduces the single one bit for bit, see
tests/test_symeigh_batched_gpu.py).  The batched back-transformation is another kernel than the single one, so the
eigenvectors are compared per kept direction by ``|<e_batched, e_immediate>| >= 1 - 1e-3`` (the criterion of
tests/test_symeig_select_gpu.py::test_select_matches_full_solver) and, for two golden cases, with the tolerances of
tests/test_api_golden.py::test_eigh.  Reference semantics: vivit/linalg/eigh.py:239-275 per group."""
import numpy as np
import pytest
import torch
from torch import nn

import vivit_amd
from helpers import FakeModule, golden_factors, load_golden, top_k_criterion
from vivit_amd.backend import backpack, extend
from vivit_amd.backend.extensions import _materialised_closures

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
DEV = torch.device("cuda:0")


def top6(evals):
    """The six largest eigenvalues, whatever their size (the early layers' curvature is tiny in absolute terms)."""
    return list(range(evals.numel() - 6, evals.numel()))


def _per_parameter_eigenpairs(model, X, y, batched):
    comp = vivit_amd.EighComputation(batched_solve=batched, warn_small_eigvals=0.0)
    groups = [{"params": [p], "criterion": top6} for p in model.parameters()]
    model.zero_grad()
    m, lossf = extend(model), extend(nn.CrossEntropyLoss())
    loss = lossf(m(X), y)
    with backpack(comp.get_extension(), extension_hook=comp.get_extension_hook(groups)):
        loss.backward()
    pending = sum(len(v) for v in comp._pending.values())
    out = [comp.get_result(g) for g in groups]
    with pytest.raises(KeyError):
        comp.get_result({"params": [], "criterion": None})
    assert all(not hasattr(p, comp._savefield) for p in model.parameters()), "save-fields must be deleted in the hook"
    return out, pending


def test_twelve_linear_layers_batched_equals_immediate():
    """12 single-parameter groups, N C = 128 * 10 = 1280: eight flushed during the pass, four on get_result."""
    torch.manual_seed(0)
    C, N = 10, 128
    layers = []
    for i in range(12):
        layers += [nn.Linear(C, C, bias=False)] + ([nn.Tanh()] if i < 11 else [])
    model = nn.Sequential(*layers).to(DEV)
    X, y = torch.rand(N, C, device=DEV), torch.randint(0, C, (N,), device=DEV)
    plain, waiting = _per_parameter_eigenpairs(model, X, y, batched=False)
    assert waiting == 0
    batched, waiting = _per_parameter_eigenpairs(model, X, y, batched=True)
    assert waiting == 4
    assert len(plain) == len(batched) == 12
    for i, ((wa, ea), (wb, eb)) in enumerate(zip(batched, plain)):
        assert wa.shape == wb.shape == (6,) and torch.equal(wa, wb), i
        assert len(ea) == len(eb) == 1 and ea[0].shape == eb[0].shape == (wa.numel(), C, C)
        dots = (ea[0].flatten(1) * eb[0].flatten(1)).sum(1).abs()
        print(f"  group {i}: K = {wa.numel()}, min |<e_batched, e_immediate>| = {dots.min().item():.7f}")
        assert (1 - dots).max().item() <= 1e-3, i
    torch.cuda.synchronize()
    assert any(not torch.equal(plain[0][0], p[0]) for p in plain[1:])


@pytest.mark.parametrize("case", ["multikernel", "mlp_small"])
def test_golden_cases_through_the_queue(case):
    """``multikernel``: n = C N = 320, a batch of one through the batched kernels; ``mlp_small``: n = 12, the looping route.
    Tolerances of tests/test_api_golden.py::test_eigh."""
    g = load_golden(case)
    V, _ = golden_factors(g, DEV)
    N, N_total = int(g["N"]), int(g["N_total"])
    sub = None if N == N_total else list(range(N))
    params = [torch.nn.Parameter(torch.zeros(*v.shape[2:], device=DEV)) for v in V]
    comp = vivit_amd.EighComputation(subsampling=sub, warn_small_eigvals=0.0, batched_solve=True)
    for p, v in zip(params, V):
        setattr(p, comp._savefield, _materialised_closures(v))
    groups = [{"params": params, "criterion": top_k_criterion(int(g["k"]))}]
    comp.get_extension_hook(groups)(FakeModule(params, N_total))
    assert sum(len(v) for v in comp._pending.values()) == 1, "the group must wait in the queue"
    assert all(not hasattr(p, comp._savefield) for p in params)
    evals, evecs = comp.get_result(groups[0])
    scale = np.abs(g["eigh_evals"]).max()
    np.testing.assert_allclose(evals.cpu().numpy(), g["eigh_evals"], rtol=1e-4, atol=1e-5 * scale)
    for i, e in enumerate(evecs):
        assert e.shape == g[f"eigh_evecs{i}"].shape
        np.testing.assert_allclose(e.abs().cpu().numpy(), np.abs(g[f"eigh_evecs{i}"]), rtol=2e-2, atol=2e-3)
    sq = sum((e.flatten(1) ** 2).sum(1) for e in evecs)
    np.testing.assert_allclose(sq.cpu().numpy(), np.ones(len(evals)), rtol=1e-5)
