"""LayerNorm and GroupNorm (with GELU and SiLU around them) in the factor provider, against the brute-force autograd oracle, and
the Computation classes end to end on models that contain them -- host and hip flavours, built as tests/test_backend.py is."""
import numpy as np
import pytest
import torch
from torch import nn

import vivit_amd
from helpers import OracleBackend, constant_damping, set_kernel_backend, top_k_criterion
from oracle import vivit_oracle as oracle
from vivit_amd.backend import BatchGrad, SqrtGGNExact, SqrtGGNMC, backpack, extend

FLAVOURS = [pytest.param("host", id="host"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]


@pytest.fixture(params=FLAVOURS)
def device(request):
    if request.param == "host":
        set_kernel_backend(OracleBackend())
        yield torch.device("cpu")
        set_kernel_backend(None)
    else:
        set_kernel_backend(None)
        yield torch.device("cuda:0")


def reinit(model):
    """Weights and biases of the normalisations away from their initial 1 and 0 (a rule that forgets gamma must show)."""
    for m in model.modules():
        if isinstance(m, (nn.LayerNorm, nn.GroupNorm)) and m.weight is not None:
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.uniform_(-0.5, 0.5)
    return model


def make_problem(name):
    torch.manual_seed(0)
    if name in ("ln_gelu_ce", "ln_noaffine_ce"):   # (a), (e)
        model = nn.Sequential(nn.Linear(7, 6), nn.LayerNorm(6, elementwise_affine=name == "ln_gelu_ce"), nn.GELU(), nn.Linear(6, 5))
        X, y, lossf, loss = torch.rand(3, 7), torch.randint(0, 5, (3,)), nn.CrossEntropyLoss(), "ce"
    elif name == "ln_extra_silu_mse":              # (b): A = 4 positions per sample
        model = nn.Sequential(nn.Linear(5, 3), nn.LayerNorm(3), nn.SiLU(), nn.Linear(3, 2), nn.Flatten())
        X, y, lossf, loss = torch.rand(3, 4, 5), torch.rand(3, 8), nn.MSELoss(), "mse"
    elif name == "gn_ce":                          # (c): G = 2, G = C and G = 1
        model = nn.Sequential(nn.Conv2d(3, 4, 2), nn.GroupNorm(2, 4), nn.GELU("tanh"), nn.Conv2d(4, 4, 2), nn.GroupNorm(4, 4), nn.Tanh(),
                              nn.GroupNorm(1, 4), nn.Flatten(), nn.Linear(36, 3))
        # (inputs from U(0, 4): a normalisation back-propagates with the factor 1 / sigma of its input, and the gradient of a bias
        # right in front of it is analytically zero -- what the oracle and the backend return there is rounding noise of the
        # size eps |M| / sigma, which inputs of a larger spread keep below the absolute tolerance of the comparison)
        X, y, lossf, loss = 4 * torch.rand(3, 3, 5, 5), torch.randint(0, 3, (3,)), nn.CrossEntropyLoss(), "ce"
    elif name == "ln_chw_ce":                      # (d): normalized_shape with several dimensions
        model = nn.Sequential(nn.Conv2d(2, 3, 2), nn.LayerNorm([3, 3, 4]), nn.Flatten(), nn.Linear(36, 3))
        X, y, lossf, loss = torch.rand(3, 2, 4, 5), torch.randint(0, 3, (3,)), nn.CrossEntropyLoss(), "ce"
    elif name == "frozen_ce":   # only one of weight and bias trainable; an eps of the module's own; GroupNorm without affine parameters
        ln, gn = nn.LayerNorm(6, eps=0.3), nn.GroupNorm(2, 6, eps=0.2)
        model = nn.Sequential(nn.Linear(7, 6), ln, nn.SiLU(), gn, nn.GroupNorm(1, 6, affine=False), nn.Linear(6, 4))
        X, y, lossf, loss = torch.rand(3, 7), torch.randint(0, 4, (3,)), nn.CrossEntropyLoss(), "ce"
        reinit(model)
        ln.weight.requires_grad_(False)
        gn.bias.requires_grad_(False)
    return reinit(model), X, y, lossf, loss


PROBLEMS = ["ln_gelu_ce", "ln_extra_silu_mse", "gn_ce", "ln_chw_ce", "ln_noaffine_ce", "frozen_ce"]


def run_backward(model, X, y, lossf, extensions, hook=None):
    model, lossf = extend(model), extend(lossf)
    model.zero_grad()
    loss = lossf(model(X), y)
    with backpack(*extensions, extension_hook=hook):
        loss.backward()
    return loss


def close(a, b, rtol=1e-4, atol=1e-6):
    np.testing.assert_allclose(a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy(), rtol=rtol, atol=atol)


def trainable(model):
    return [p for p in model.parameters() if p.requires_grad]


@pytest.mark.parametrize("subsampling", [None, [0, 0, 1, 0, 1]], ids=["full", "repeated"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_sqrt_ggn_and_batch_grad_factors(problem, subsampling, device):
    model, X, y, lossf, loss = make_problem(problem)
    ref_model, _, _, ref_lossf, _ = make_problem(problem)
    S = oracle.loss_hessian_sqrt_exact(ref_model(X).detach(), loss)
    V_ref = oracle.sqrt_ggn_factors(ref_model, X, S, subsampling)
    g_ref = oracle.batch_grads(ref_model, X, y, ref_lossf, subsampling)
    assert len(V_ref) == len(g_ref) == len(trainable(ref_model))

    model, X, y = model.to(device), X.to(device), y.to(device)
    run_backward(model, X, y, lossf, [SqrtGGNExact(subsampling=subsampling), BatchGrad(subsampling=subsampling)])
    for p, v, g in zip(trainable(model), V_ref, g_ref):
        close(p.sqrt_ggn_exact, v, rtol=1e-4, atol=1e-6)
        close(p.grad_batch, g, rtol=1e-4, atol=1e-7)


def test_mc_factors_with_supplied_samples(device):
    model, X, y, lossf, loss = make_problem("ln_gelu_ce")
    ref_model = make_problem("ln_gelu_ce")[0]
    out = ref_model(X).detach()
    gen = torch.Generator().manual_seed(1)
    idx = torch.multinomial(out.softmax(1), 3, replacement=True, generator=gen)
    onehots = torch.nn.functional.one_hot(idx.t(), out.shape[1]).to(out.dtype)
    V_ref = oracle.sqrt_ggn_factors(ref_model, X, oracle.loss_hessian_sqrt_mc(out, onehots))
    model, X, y = model.to(device), X.to(device), y.to(device)
    run_backward(model, X, y, lossf, [SqrtGGNMC(mc_samples=3, samples=onehots)])
    for p, v in zip(model.parameters(), V_ref):
        close(p.sqrt_ggn_mc, v, rtol=1e-4, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("problem", PROBLEMS)
def test_rules_run_on_the_hip_kernels(problem, monkeypatch):
    """On the GPU no rule of these models may reach ``torch.autograd.grad`` (the generic input rule), ``torch.einsum`` or
    ``torch.func.vmap``: LayerNorm, GroupNorm, GELU and SiLU are launches of the HIP kernels."""

    def forbidden(*a, **k):
        raise AssertionError("fell back to the torch rule")

    set_kernel_backend(None)
    dev = torch.device("cuda:0")
    model, X, y, lossf, loss = make_problem(problem)
    ref_model = make_problem(problem)[0]
    S = oracle.loss_hessian_sqrt_exact(ref_model(X).detach(), loss)
    V_ref = oracle.sqrt_ggn_factors(ref_model, X, S, None)
    model, X, y = model.to(dev), X.to(dev), y.to(dev)
    monkeypatch.setattr(torch, "einsum", forbidden)
    monkeypatch.setattr(torch.autograd, "grad", forbidden)
    monkeypatch.setattr(torch.func, "vmap", forbidden)
    run_backward(model, X, y, lossf, [SqrtGGNExact()])
    monkeypatch.undo()
    for p, v in zip(trainable(model), V_ref):
        close(p.sqrt_ggn_exact, v, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("groups_kind", ["one", "per_parameter"])
@pytest.mark.parametrize("problem", ["ln_gelu_ce", "gn_ce"])
def test_eigvalsh_and_eigh_end_to_end(problem, groups_kind, device):
    """Gram eigenvalues == dense-GGN eigenvalues on the top min(n, P); G e = lambda e; orthonormal -- as
    tests/test_backend.py::test_eigvalsh_and_eigh_end_to_end, with one group and with one group per parameter."""
    model, X, y, lossf, loss = make_problem(problem)
    ref_model = make_problem(problem)[0].double()
    named = list(ref_model.named_parameters())
    model, X, y = model.to(device), X.to(device), y.to(device)
    params = list(model.parameters())
    index_groups = [list(range(len(params)))] if groups_kind == "one" else [[i] for i in range(len(params))]
    ggn = oracle.dense_ggn(ref_model, X.double().cpu(), loss)
    offs = np.cumsum([0] + [p.numel() for _, p in named])

    def block(idx):
        sel = np.concatenate([np.arange(offs[i], offs[i + 1]) for i in idx])
        return ggn[sel][:, sel]

    comp = vivit_amd.EigvalshComputation()
    groups = [{"params": [params[i] for i in idx]} for idx in index_groups]
    run_backward(model, X, y, lossf, [comp.get_extension()], comp.get_extension_hook(groups))
    for idx, grp in zip(index_groups, groups):
        ref_w = torch.linalg.eigvalsh(block(idx))
        w = comp.get_result(grp).cpu().double()
        k = min(len(w), len(ref_w))
        np.testing.assert_allclose(w[-k:].numpy(), ref_w[-k:].numpy(), rtol=1e-4, atol=5e-6)

    comp = vivit_amd.EighComputation(warn_small_eigvals=0.0)
    crit = lambda evals: [i for i in range(evals.numel()) if evals[i].abs() >= max(1e-4, 1e-3 * float(evals[-1]))]   # noqa: E731
    # (a bias right in front of a normalisation over its own channel alone -- Conv2d before GroupNorm(4, 4) -- has a GGN block
    # that is exactly zero: the criterion selects no direction there and the reference has no eigenpair to compare with)
    index_groups = [idx for idx in index_groups if float(torch.linalg.eigvalsh(block(idx))[-1]) >= 1e-4]
    assert len(index_groups) >= (1 if groups_kind == "one" else len(params) - 1)
    groups = [{"params": [params[i] for i in idx], "criterion": crit} for idx in index_groups]
    run_backward(model, X, y, lossf, [comp.get_extension()], comp.get_extension_hook(groups))
    for idx, grp in zip(index_groups, groups):
        evals, evecs = comp.get_result(grp)
        assert evals.numel() > 0
        E = torch.cat([e.flatten(1) for e in evecs], 1).cpu().double()
        B = block(idx)
        np.testing.assert_allclose((E @ E.T).numpy(), np.eye(E.shape[0]), atol=2e-4)
        np.testing.assert_allclose((E @ B).numpy(), (evals.cpu().double()[:, None] * E).numpy(), rtol=1e-3, atol=2e-4)


@pytest.mark.parametrize("problem", ["ln_gelu_ce", "gn_ce"])
def test_damped_newton_end_to_end(problem, device):
    """Newton step == the oracle's restatement on autograd factors, as tests/test_backend.py::test_damped_newton_end_to_end."""
    model, X, y, lossf, loss = make_problem(problem)
    ref_model, _, _, ref_lossf, _ = make_problem(problem)
    out = ref_model(X).detach()
    N = out.shape[0]
    V_ref = oracle.sqrt_ggn_factors(ref_model, X, oracle.loss_hessian_sqrt_exact(out, loss), None)
    g_ref = oracle.batch_grads(ref_model, X, y, ref_lossf, None)
    crit = top_k_criterion(3, must_exceed=1e-4)
    ref_steps = oracle.damped_newton_group(V_ref, g_ref, crit, constant_damping(1.0), N)

    model, X, y = model.to(device), X.to(device), y.to(device)
    comp = vivit_amd.DirectionalDampedNewtonComputation(warn_small_eigvals=0.0)
    groups = [{"params": list(model.parameters()), "criterion": crit, "damping": constant_damping(1.0)}]
    run_backward(model, X, y, lossf, comp.get_extensions(), comp.get_extension_hook(groups))
    for s, r in zip(comp.get_result(groups[0]), ref_steps):
        close(s, r, rtol=1e-3, atol=2e-5 * max(r.abs().max().item(), 1e-2))
