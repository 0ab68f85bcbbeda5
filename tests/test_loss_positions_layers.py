"""Losses on outputs with positions -- ``nn.CrossEntropyLoss`` and ``nn.MSELoss`` on ``[N, C, *D]`` -- and the ``Permute`` module in
the factor provider, against the brute-force autograd oracle and a dense fp64 restatement, host and hip flavours (the fixture of
tests/test_llama_layers.py, copied).  Tolerances: those of tests/test_llama_layers.py, unchanged.

On the commit before this capability every ``SqrtGGN*`` case fails with "loss input must be [N, C]", and the file itself at the
import of ``Permute``."""
import math

import numpy as np
import pytest
import torch
from torch import nn

import loss_positions_refs as refs
import vivit_amd
from helpers import OracleBackend, constant_damping, set_kernel_backend, top_k_criterion
from oracle import vivit_oracle as oracle
from vivit_amd.backend import (ActiveIdentity, BatchGrad, Parallel, Permute, ProductModule, RotaryEmbedding, ScaledDotProductAttention,
                               SqrtGGNExact, SqrtGGNMC, ViViTGGNExact, backpack, extend)

FLAVOURS = [pytest.param("host", id="host"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
F64 = torch.float64


@pytest.fixture(params=FLAVOURS)
def device(request):
    if request.param == "host":
        set_kernel_backend(OracleBackend())
        yield torch.device("cpu")
        set_kernel_backend(None)
    else:
        set_kernel_backend(None)
        yield torch.device("cuda:0")


class IdsFromFloat(nn.Module):
    """Float token ids -> int64 (the oracle's side only, as tests/test_embedding_layers.py)."""

    def forward(self, x):
        return x.round().long()


def reinit(model):
    """Weights of the RMSNorms away from their initial 1 (a rule that forgets gamma must show)."""
    for m in model.modules():
        if isinstance(m, nn.RMSNorm) and m.weight is not None:
            m.weight.data.uniform_(0.5, 1.5)
    return model


def swiglu(E, F_):
    return Parallel(nn.Sequential(nn.Linear(E, F_), nn.SiLU()), nn.Linear(E, F_), merge_module=ProductModule())


def make_problem(name):
    torch.manual_seed(0)
    if name == "linear_permute_ce":      # (a): a head on [N, T, in], classes moved to axis 1: rows of classes per position
        model = nn.Sequential(nn.Linear(6, 4), Permute(0, 2, 1))
        X, y, lossf, loss = torch.rand(3, 5, 6), torch.randint(0, 4, (3, 5)), nn.CrossEntropyLoss(), "ce"
    elif name == "conv2d_ce":            # (b): segmentation, [N, C, H, W] = [3, 3, 3, 4] straight from the convolution
        model = nn.Sequential(nn.Conv2d(2, 3, 2))
        X, y, lossf, loss = torch.rand(3, 2, 4, 5), torch.randint(0, 3, (3, 3, 4)), nn.CrossEntropyLoss(), "ce"
    elif name == "conv1d_mse":           # (c): dense regression on [3, 2, 4]
        model = nn.Sequential(nn.Conv1d(3, 2, 2))
        X, y, lossf, loss = torch.rand(3, 3, 5), torch.rand(3, 2, 4), nn.MSELoss(), "mse"
    elif name == "decoder_lm_ce":        # (d): the decoder block of tests/test_llama_layers.py on embedded tokens, next-token
        E, H = 8, 2                      #      cross entropy over all T = 5 positions
        attention = nn.Sequential(nn.RMSNorm(E, eps=1e-5), nn.Linear(E, 3 * E), RotaryEmbedding(H), ScaledDotProductAttention(H, causal=True),
                                  nn.Linear(E, E))
        mlp = nn.Sequential(nn.RMSNorm(E, eps=1e-5), swiglu(E, 12), nn.Linear(12, E))
        model = nn.Sequential(nn.Embedding(11, E), Parallel(ActiveIdentity(), attention), Parallel(ActiveIdentity(), mlp),
                              nn.RMSNorm(E, eps=1e-5), nn.Linear(E, 3), Permute(0, 2, 1))
        X = torch.tensor([[1, 4, 1, 7, 2], [4, 2, 9, 10, 0], [0, 3, 5, 5, 8]])
        y, lossf, loss = torch.randint(0, 3, (3, 5)), nn.CrossEntropyLoss(), "ce"
        reinit(model)
        model[-2].weight.data.mul_(0.25)   # (as tests/test_llama_layers.py scales its head: spectra of order one)
    return model, X, y, lossf, loss


PROBLEMS = ["linear_permute_ce", "conv2d_ce", "conv1d_mse", "decoder_lm_ce"]
LM_PROBLEMS = ["linear_permute_ce", "decoder_lm_ce"]


def make_reference(name):
    """The same model in fp64 (token ids behind :class:`IdsFromFloat`) and its float input."""
    model, X, y, lossf, loss = make_problem(name)
    if not X.is_floating_point():
        model = nn.Sequential(IdsFromFloat(), *model)
    return model.double(), X.double(), y.double() if y.is_floating_point() else y, lossf, loss


def run_backward(model, X, y, lossf, extensions, hook=None):
    model, lossf = extend(model), extend(lossf)
    model.zero_grad()
    loss = lossf(model(X), y)
    with backpack(*extensions, extension_hook=hook):
        loss.backward()
    return loss


def close(a, b, rtol=1e-4, atol=1e-6):
    np.testing.assert_allclose(a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy(), rtol=rtol, atol=atol)


@pytest.mark.parametrize("subsampling", [None, [2, 0]], ids=["full", "subsampled"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_sqrt_ggn_and_batch_grad_factors(problem, subsampling, device):
    model, X, y, lossf, loss = make_problem(problem)
    ref_model, Xf, yf, ref_lossf, _ = make_reference(problem)
    S_ref = refs.exact_factor(ref_model(Xf).detach(), loss)
    V_ref = oracle.sqrt_ggn_factors(ref_model, Xf, S_ref.flatten(2), subsampling)
    g_ref = oracle.batch_grads(ref_model, Xf, yf, ref_lossf, subsampling)
    assert len(V_ref) == len(g_ref) == len(list(model.parameters()))
    assert all(float(v.abs().max()) > 1e-3 for v in V_ref)

    model, X, y = model.to(device), X.to(device), y.to(device)
    run_backward(model, X, y, lossf, [SqrtGGNExact(subsampling=subsampling), BatchGrad(subsampling=subsampling)])
    for p, v, g in zip(model.parameters(), V_ref, g_ref):
        close(p.sqrt_ggn_exact, v, rtol=1e-4, atol=1e-6)
        close(p.grad_batch, g, rtol=1e-4, atol=1e-7)


def supplied_samples(out, loss, M=3):
    """(samples to hand to SqrtGGNMC, the reference factor) for the output ``out [N, C, *D]`` (fp64)."""
    N, C, D = out.shape[0], out.shape[1], tuple(out.shape[2:])
    L = math.prod(D)
    gen = torch.Generator().manual_seed(1)
    if loss == "ce":
        draws = torch.multinomial(out.softmax(1).movedim(1, -1).reshape(N * L, C), M, replacement=True, generator=gen)
        idx = draws.t().reshape(M, N, *D)
        return idx, refs.ce_sampled(out, idx, 1.0 / math.sqrt(M * N * L))
    eps = torch.randn(M, *out.shape, generator=gen)
    return eps, refs.mse_sampled(eps, math.sqrt(2.0 / (M * N * C * L)))


@pytest.mark.parametrize("subsampling", [None, [2, 0]], ids=["full", "subsampled"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_mc_factors_with_supplied_samples(problem, subsampling, device):
    """Supplied samples: class indices [M, N, *D] for the cross entropy, standard-normal draws for the squared error."""
    model, X, y, lossf, loss = make_problem(problem)
    ref_model, Xf, _, _, _ = make_reference(problem)
    samples, S_ref = supplied_samples(ref_model(Xf).detach(), loss)
    V_ref = oracle.sqrt_ggn_factors(ref_model, Xf, S_ref.flatten(2), subsampling)
    model, X, y = model.to(device), X.to(device), y.to(device)
    run_backward(model, X, y, lossf, [SqrtGGNMC(mc_samples=3, samples=samples, subsampling=subsampling)])
    for p, v in zip(model.parameters(), V_ref):
        close(p.sqrt_ggn_mc, v, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("problem", ["linear_permute_ce", "conv2d_ce"])
def test_one_hot_samples_are_reduced_to_indices(problem, device):
    model, X, y, lossf, loss = make_problem(problem)
    ref_model, Xf, _, _, _ = make_reference(problem)
    out = ref_model(Xf).detach()
    idx, _ = supplied_samples(out, loss)
    onehots = torch.nn.functional.one_hot(idx, out.shape[1]).movedim(-1, 2).float()      # [M, N, C, *D]
    model, X, y = model.to(device), X.to(device), y.to(device)
    run_backward(model, X, y, lossf, [SqrtGGNMC(mc_samples=3, samples=idx)])
    from_indices = [p.sqrt_ggn_mc.clone() for p in model.parameters()]
    run_backward(model, X, y, lossf, [SqrtGGNMC(mc_samples=3, samples=onehots)])
    for p, v in zip(model.parameters(), from_indices):
        assert torch.equal(p.sqrt_ggn_mc, v)


def test_drawn_samples_have_the_documented_shapes(device):
    """No samples supplied: indices are drawn from the softmax at every position (cross entropy), normal draws (squared error)."""
    for problem in ("linear_permute_ce", "conv1d_mse"):
        model, X, y, lossf, _ = make_problem(problem)
        model, X, y = model.to(device), X.to(device), y.to(device)
        run_backward(model, X, y, lossf, [SqrtGGNMC(mc_samples=2)])
        for p in model.parameters():
            assert p.sqrt_ggn_mc.shape == (2, 3) + tuple(p.shape) and bool(torch.isfinite(p.sqrt_ggn_mc).all())


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("problem", ["linear_permute_ce", "conv1d_mse"])
def test_reductions(problem, reduction, device):
    model, X, y, _, loss = make_problem(problem)
    ref_model, Xf, _, _, _ = make_reference(problem)
    lossf = (nn.CrossEntropyLoss if loss == "ce" else nn.MSELoss)(reduction=reduction)
    S_ref = refs.exact_factor(ref_model(Xf).detach(), loss, reduction)
    V_ref = oracle.sqrt_ggn_factors(ref_model, Xf, S_ref.flatten(2), None)
    model, X, y = model.to(device), X.to(device), y.to(device)
    run_backward(model, X, y, lossf, [SqrtGGNExact()])
    for p, v in zip(model.parameters(), V_ref):
        close(p.sqrt_ggn_exact, v, rtol=1e-4, atol=1e-6)


# ---- the Computation classes end to end, against a dense fp64 restatement ---------------------------------------------------------
def dense_reference(problem):
    """(GGN [P, P], gradient [P], parameter shapes) of the mini-batch loss in fp64: the GGN from per-sample Jacobians and the autograd
    Hessian of the REAL loss w.r.t. each sample's output, the gradient from autograd."""
    ref_model, Xf, yf, lossf, _ = make_reference(problem)
    params = [p for p in ref_model.parameters() if p.requires_grad]
    jac = oracle.per_sample_jacobians(ref_model, Xf)                                # [N, C L, *param]
    out = ref_model(Xf).detach()
    N, K = out.shape[0], out[0].numel()
    J = torch.cat([j.reshape(N, K, -1) for j in jac], dim=2)                        # [N, C L, P]
    ggn = torch.zeros(J.shape[2], J.shape[2], dtype=F64)
    for n in range(N):
        def f(o):
            return lossf(torch.cat((out[:n], o.unsqueeze(0), out[n + 1:])), yf)

        H = torch.autograd.functional.hessian(f, out[n].clone()).reshape(K, K)
        ggn += J[n].T @ H @ J[n]
    grads = torch.autograd.grad(lossf(ref_model(Xf), yf), params)
    return ggn, torch.cat([g.flatten() for g in grads]), [p.shape for p in params]


@pytest.mark.parametrize("problem", LM_PROBLEMS)
def test_eigh_end_to_end(problem, device):
    """Gram eigenvalues == the top dense-GGN eigenvalues; G e = lambda e; orthonormal (tolerances of
    tests/test_llama_layers.py::test_eigvalsh_and_eigh_end_to_end)."""
    ggn, _, _ = dense_reference(problem)
    model, X, y, lossf, _ = make_problem(problem)
    model, X, y = model.to(device), X.to(device), y.to(device)
    crit = top_k_criterion(3, must_exceed=1e-4)
    comp = vivit_amd.EighComputation(warn_small_eigvals=0.0)
    group = {"params": list(model.parameters()), "criterion": crit}
    run_backward(model, X, y, lossf, [comp.get_extension()], comp.get_extension_hook([group]))
    evals, evecs = comp.get_result(group)
    ref_w = torch.linalg.eigvalsh(ggn)
    assert evals.numel() == 3
    np.testing.assert_allclose(evals.cpu().double().numpy(), ref_w[-3:].numpy(), rtol=1e-4, atol=5e-6)
    E = torch.cat([e.flatten(1) for e in evecs], 1).cpu().double()
    np.testing.assert_allclose((E @ E.T).numpy(), np.eye(3), atol=2e-4)
    np.testing.assert_allclose((E @ ggn).numpy(), (evals.cpu().double()[:, None] * E).numpy(), rtol=1e-3, atol=2e-4)


@pytest.mark.parametrize("problem", LM_PROBLEMS)
def test_damped_newton_end_to_end(problem, device):
    """Newton step == - sum_k gamma_k / (lambda_k + delta) e_k over the top three eigenvectors of the dense GGN, gamma_k = g^T e_k (the
    sqrt(N) / N compensation of the optim classes holds for a per-sample loss that is a mean over positions); tolerances of
    tests/test_llama_layers.py::test_damped_newton_end_to_end."""
    ggn, grad, shapes = dense_reference(problem)
    w, Q = torch.linalg.eigh(ggn)
    keep = top_k_criterion(3, must_exceed=1e-4)(w)
    assert len(keep) == 3
    step = torch.zeros_like(grad)
    for k in keep:
        step -= (grad @ Q[:, k]) / (w[k] + 1.0) * Q[:, k]
    ref_steps, off = [], 0
    for shp in shapes:
        ref_steps.append(step[off:off + math.prod(shp)].reshape(shp))
        off += math.prod(shp)

    model, X, y, lossf, _ = make_problem(problem)
    model, X, y = model.to(device), X.to(device), y.to(device)
    comp = vivit_amd.DirectionalDampedNewtonComputation(warn_small_eigvals=0.0)
    groups = [{"params": list(model.parameters()), "criterion": top_k_criterion(3, must_exceed=1e-4), "damping": constant_damping(1.0)}]
    run_backward(model, X, y, lossf, comp.get_extensions(), comp.get_extension_hook(groups))
    for s, r in zip(comp.get_result(groups[0]), ref_steps):
        close(s, r, rtol=1e-3, atol=2e-5 * max(r.abs().max().item(), 1e-2))


def test_vivit_ggn_closures_gram_equals_the_gram_of_the_factors(device):
    model, X, y, lossf, _ = make_problem("linear_permute_ce")
    model, X, y = model.to(device), X.to(device), y.to(device)
    run_backward(model, X, y, lossf, [SqrtGGNExact(), ViViTGGNExact()])
    for p in model.parameters():
        V = p.sqrt_ggn_exact.flatten(2).cpu().double()                              # [C L, N, P]
        G = torch.einsum("vnp,wmp->vnwm", V, V)
        close(p.vivit_ggn_exact["gram_mat"](), G, rtol=1e-4, atol=1e-6)


@pytest.mark.gpu
def test_the_language_model_runs_on_the_hip_kernels(monkeypatch):
    """On the GPU the extension pass of the decoder with the per-position loss reaches neither ``torch.autograd.grad`` (the generic
    input rule) nor ``torch.func.vmap``: the loss factor, Permute and every layer below are kernels or views."""

    def forbidden(*a, **k):
        raise AssertionError("fell back to the torch rule")

    set_kernel_backend(None)
    dev = torch.device("cuda:0")
    problem = "decoder_lm_ce"
    model, X, y, lossf, loss = make_problem(problem)
    ref_model, Xf, _, _, _ = make_reference(problem)
    S_ref = refs.exact_factor(ref_model(Xf).detach(), loss)
    V_ref = oracle.sqrt_ggn_factors(ref_model, Xf, S_ref.flatten(2), None)
    idx, S_mc = supplied_samples(ref_model(Xf).detach(), loss)
    V_mc = oracle.sqrt_ggn_factors(ref_model, Xf, S_mc.flatten(2), None)
    model, X, y = model.to(dev), X.to(dev), y.to(dev)
    monkeypatch.setattr(torch.autograd, "grad", forbidden)
    monkeypatch.setattr(torch.func, "vmap", forbidden)
    run_backward(model, X, y, lossf, [SqrtGGNExact(), SqrtGGNMC(mc_samples=3, samples=idx)])
    monkeypatch.undo()
    for p, v, m in zip(model.parameters(), V_ref, V_mc):
        close(p.sqrt_ggn_exact, v, rtol=1e-4, atol=1e-6)
        close(p.sqrt_ggn_mc, m, rtol=1e-4, atol=1e-6)


@pytest.mark.gpu
def test_the_factor_below_permute_is_contiguous():
    """The kernel writes the factor in the memory format of the permuted logits: Permute's rule hands the head a contiguous tensor."""
    from vivit_amd.backend import extensions

    set_kernel_backend(None)
    dev = torch.device("cuda:0")
    model, X, y, lossf, _ = make_problem("linear_permute_ce")
    model, lossf = extend(model.to(dev)), extend(lossf)
    lossf(model(X.to(dev)), y.to(dev))
    S = extensions._loss_hessian_sqrt(lossf, "exact", 1, None)
    assert S.shape == (20, 3, 4, 5) and not S.is_contiguous()
    M = extensions._jac_t_mat_prod(model[1], S, model[1].input0.detach())
    assert M.shape == (20, 3, 5, 4) and M.is_contiguous() and M.data_ptr() == S.data_ptr()


# ---- Permute itself ---------------------------------------------------------------------------------------------------------------------
def test_permute_module():
    for dims in [(1, 0), (0, 0, 1), (0, 3, 1), (), (0, 1.0), (1, 2, 0)]:
        with pytest.raises(ValueError):
            Permute(*dims)
    x = torch.rand(2, 3, 4, 5)
    mod = Permute(0, 2, 3, 1)
    assert torch.equal(mod(x), x.permute(0, 2, 3, 1)) and mod(x).shape == (2, 4, 5, 3)
    assert torch.equal(Permute((0, 2, 1))(x[0]), x[0].permute(0, 2, 1))       # (dims as one sequence)
    assert torch.equal(Permute(0, 1, 2, 3)(x), x)
    assert list(mod.parameters()) == []
    assert "Permute" in vivit_amd.backend.__all__


def test_permute_rule_is_a_view_of_the_factor():
    from vivit_amd.backend import extensions

    x = torch.rand(2, 3, 4, 5)
    mod = Permute(0, 2, 3, 1)
    M = torch.rand(6, 2, 4, 5, 3)                                                 # [V, N, *out]
    g = extensions._jac_t_mat_prod(mod, M, x)
    assert g.shape == (6, 2, 3, 4, 5)
    assert g.untyped_storage().data_ptr() == M.untyped_storage().data_ptr() and not g.requires_grad
    assert torch.equal(g, extensions._generic_jac_t_mat_prod(mod, M, x))          # the transposed Jacobian, by autograd
    assert torch.equal(g, M.permute(0, 1, 4, 2, 3))


# ---- the [N, C] path is what it was ---------------------------------------------------------------------------------------------------
def flat_problem(device):
    from vivit_amd.backend import extensions

    torch.manual_seed(0)
    model, lossf = extend(nn.Sequential(nn.Linear(7, 5)).to(device)), extend(nn.CrossEntropyLoss())
    lossf(model(torch.rand(3, 7, device=device)), torch.randint(0, 5, (3,), device=device))
    onehots = torch.nn.functional.one_hot(torch.randint(0, 5, (2, 3)), 5).float()
    return extensions, lossf, lossf.input0.detach(), onehots


def test_flat_outputs_take_the_flat_formulas():
    extensions, lossf, out, onehots = flat_problem(torch.device("cpu"))
    close(extensions._loss_hessian_sqrt(lossf, "exact", 1, None), oracle.loss_hessian_sqrt_exact(out, "ce"), rtol=1e-6, atol=1e-8)
    close(extensions._loss_hessian_sqrt(lossf, "sampling", 2, onehots), oracle.loss_hessian_sqrt_mc(out, onehots), rtol=1e-6, atol=1e-8)


@pytest.mark.gpu
def test_flat_outputs_take_the_flat_kernel_bit_for_bit():
    from vivit_amd import kernels

    set_kernel_backend(None)
    dev = torch.device("cuda:0")
    extensions, lossf, out, onehots = flat_problem(dev)
    assert torch.equal(extensions._loss_hessian_sqrt(lossf, "exact", 1, None), kernels.ce_sqrt_hessian(out, 1.0 / math.sqrt(3)))
    assert torch.equal(extensions._loss_hessian_sqrt(lossf, "sampling", 2, onehots),
                       kernels.ce_sqrt_hessian(out, 1.0 / math.sqrt(2 * 3), onehot=onehots.to(dev)))
