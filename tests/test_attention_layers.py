"""Multi-head self-attention in the factor provider, against the brute-force autograd oracle, and the Computation classes end to end on
a model that contains it -- host and hip flavours, built as tests/test_norm_layers.py is."""
import numpy as np
import pytest
import torch
from torch import nn

import vivit_amd
from helpers import OracleBackend, constant_damping, set_kernel_backend, top_k_criterion
from oracle import vivit_oracle as oracle
from vivit_amd.backend import (
    ActiveIdentity,
    BatchGrad,
    MultiheadSelfAttention,
    Parallel,
    ScaledDotProductAttention,
    Slicing,
    SqrtGGNExact,
    SqrtGGNMC,
    backpack,
    extend,
)

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
    """Every weight and bias away from symmetric or trivial values (LayerNorm's 1 and 0, zero biases of the projections)."""
    g = torch.Generator().manual_seed(1)
    for p in model.parameters():
        p.data.copy_(torch.rand(p.shape, generator=g) * 1.2 - 0.5)
    for m in model.modules():
        if isinstance(m, nn.LayerNorm):
            m.weight.data.add_(1.0)
    return model


def make_problem(name):
    torch.manual_seed(0)
    if name == "sdpa_ce":            # (a)
        model = nn.Sequential(nn.Linear(6, 18), ScaledDotProductAttention(2), nn.Linear(6, 6), nn.Flatten(), nn.Linear(24, 5))
        X, y, lossf, loss = torch.rand(3, 4, 6), torch.randint(0, 5, (3,)), nn.CrossEntropyLoss(), "ce"
    elif name == "encoder_mse":      # (b): a pre-LN residual encoder block with causal attention, class-token pooling
        E = 8
        model = nn.Sequential(
            Parallel(ActiveIdentity(), nn.Sequential(nn.LayerNorm(E), MultiheadSelfAttention(E, 2, causal=True))),
            Parallel(ActiveIdentity(), nn.Sequential(nn.LayerNorm(E), nn.Linear(E, 12), nn.GELU(), nn.Linear(12, E))),
            Slicing((slice(None), 0)), nn.Linear(E, 3))
        X, y, lossf, loss = torch.rand(3, 5, E), torch.rand(3, 3), nn.MSELoss(), "mse"
    elif name == "odd_ce":           # (c): H = 1, d = E = 5, T = 7
        model = nn.Sequential(nn.Linear(3, 15), ScaledDotProductAttention(1), nn.Flatten(), nn.Linear(35, 4))
        X, y, lossf, loss = torch.rand(3, 7, 3), torch.randint(0, 4, (3,)), nn.CrossEntropyLoss(), "ce"
    return reinit(model), X, y, lossf, loss


PROBLEMS = ["sdpa_ce", "encoder_mse", "odd_ce"]


def run_backward(model, X, y, lossf, extensions, hook=None):
    model, lossf = extend(model), extend(lossf)
    model.zero_grad()
    loss = lossf(model(X), y)
    with backpack(*extensions, extension_hook=hook):
        loss.backward()
    return loss


def close(a, b, rtol=1e-4, atol=1e-6):
    np.testing.assert_allclose(a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy(), rtol=rtol, atol=atol)


# ("permuted" has the batch's length: an output that was not sub-sampled would have the right shape and the wrong rows)
@pytest.mark.parametrize("subsampling", [None, [0, 0, 1, 0, 1], [2, 0, 1]], ids=["full", "repeated", "permuted"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_sqrt_ggn_and_batch_grad_factors(problem, subsampling, device):
    model, X, y, lossf, loss = make_problem(problem)
    ref_model, _, _, ref_lossf, _ = make_problem(problem)
    S = oracle.loss_hessian_sqrt_exact(ref_model(X).detach(), loss)
    V_ref = oracle.sqrt_ggn_factors(ref_model, X, S, subsampling)
    g_ref = oracle.batch_grads(ref_model, X, y, ref_lossf, subsampling)
    assert len(V_ref) == len(g_ref) == len(list(ref_model.parameters()))

    model, X, y = model.to(device), X.to(device), y.to(device)
    run_backward(model, X, y, lossf, [SqrtGGNExact(subsampling=subsampling), BatchGrad(subsampling=subsampling)])
    for p, v, g in zip(model.parameters(), V_ref, g_ref):
        close(p.sqrt_ggn_exact, v, rtol=1e-4, atol=1e-6)
        close(p.grad_batch, g, rtol=1e-4, atol=1e-7)


def test_mc_factors_with_supplied_samples(device):
    model, X, y, lossf, loss = make_problem("sdpa_ce")
    ref_model = make_problem("sdpa_ce")[0]
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
def test_encoder_block_runs_on_the_hip_kernels(monkeypatch):
    """On the GPU no rule of the encoder block may reach ``torch.autograd.grad`` (the generic input rule), ``torch.einsum`` or
    ``torch.func.vmap``: attention is a launch of the HIP kernel, as LayerNorm, GELU, Linear and the index modules are."""

    def forbidden(*a, **k):
        raise AssertionError("fell back to the torch rule")

    set_kernel_backend(None)
    dev = torch.device("cuda:0")
    model, X, y, lossf, loss = make_problem("encoder_mse")
    ref_model = make_problem("encoder_mse")[0]
    S = oracle.loss_hessian_sqrt_exact(ref_model(X).detach(), loss)
    V_ref = oracle.sqrt_ggn_factors(ref_model, X, S, None)
    model, X, y = model.to(dev), X.to(dev), y.to(dev)
    monkeypatch.setattr(torch, "einsum", forbidden)
    monkeypatch.setattr(torch.autograd, "grad", forbidden)
    monkeypatch.setattr(torch.func, "vmap", forbidden)
    run_backward(model, X, y, lossf, [SqrtGGNExact()])
    monkeypatch.undo()
    for p, v in zip(model.parameters(), V_ref):
        close(p.sqrt_ggn_exact, v, rtol=1e-4, atol=1e-6)


def test_eigh_end_to_end(device):
    """G e = lambda e and orthonormality against the dense GGN, as tests/test_norm_layers.py::test_eigvalsh_and_eigh_end_to_end."""
    model, X, y, lossf, loss = make_problem("sdpa_ce")
    ref_model = make_problem("sdpa_ce")[0].double()
    model, X, y = model.to(device), X.to(device), y.to(device)
    ggn = oracle.dense_ggn(ref_model, X.double().cpu(), loss)
    comp = vivit_amd.EighComputation(warn_small_eigvals=0.0)
    crit = lambda evals: [i for i in range(evals.numel()) if evals[i].abs() >= max(1e-4, 1e-3 * float(evals[-1]))]   # noqa: E731
    groups = [{"params": list(model.parameters()), "criterion": crit}]
    run_backward(model, X, y, lossf, [comp.get_extension()], comp.get_extension_hook(groups))
    evals, evecs = comp.get_result(groups[0])
    assert evals.numel() > 0
    E = torch.cat([e.flatten(1) for e in evecs], 1).cpu().double()
    np.testing.assert_allclose((E @ E.T).numpy(), np.eye(E.shape[0]), atol=2e-4)
    np.testing.assert_allclose((E @ ggn).numpy(), (evals.cpu().double()[:, None] * E).numpy(), rtol=1e-3, atol=2e-4)


def test_damped_newton_end_to_end(device):
    """Newton step == the oracle's restatement on autograd factors, as tests/test_norm_layers.py::test_damped_newton_end_to_end."""
    model, X, y, lossf, loss = make_problem("sdpa_ce")
    ref_model, _, _, ref_lossf, _ = make_problem("sdpa_ce")
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


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("bias", [True, False])
def test_from_torch_reproduces_multihead_attention(causal, bias):
    torch.manual_seed(3)
    E, H, T = 12, 3, 6
    mha = nn.MultiheadAttention(E, H, bias=bias, batch_first=True).double()
    if bias:
        mha.in_proj_bias.data.uniform_(-0.5, 0.5)
        mha.out_proj.bias.data.uniform_(-0.5, 0.5)
    ours = MultiheadSelfAttention.from_torch(mha, causal=causal)
    x = torch.randn(4, T, E, dtype=torch.float64)
    mask = torch.ones(T, T, dtype=torch.bool).triu(1) if causal else None
    ref = mha(x, x, x, need_weights=False, attn_mask=mask)[0]
    got = ours(x)
    assert got.shape == ref.shape
    assert ((got - ref).abs().max() / ref.abs().max()).item() <= 1e-12


def test_output_of_another_batch_is_refused(device):
    """The rule reads the forward output from the module.  One that does not belong to the input after sub-sampling (here: left
    un-sub-sampled, three rows against five) is an error, not a silently recomputed forward."""
    from vivit_amd.backend.extensions import _jac_t_mat_prod

    torch.manual_seed(2)
    module = ScaledDotProductAttention(2)
    x = torch.rand(3, 4, 12, device=device)
    module.output = module(x)
    sub = [0, 0, 1, 0, 1]
    M = torch.rand(2, 5, 4, 4, device=device)
    got = _jac_t_mat_prod(module, M, x[sub], sub)
    module.output = None                                             # (a module called outside the engine: one forward)
    close(got, _jac_t_mat_prod(module, M, x[sub], sub), rtol=1e-5, atol=1e-7)
    module.output = module(x)
    with pytest.raises(ValueError):
        _jac_t_mat_prod(module, M, x[sub])
    module.output = module(x).double()
    with pytest.raises(ValueError):
        _jac_t_mat_prod(module, M, x[sub], sub)


def test_input_validation():
    with pytest.raises(ValueError):
        ScaledDotProductAttention(2)(torch.rand(4, 12))           # not [N, T, 3 E]
    with pytest.raises(ValueError):
        ScaledDotProductAttention(2)(torch.rand(3, 4, 15))        # 15 is not 3 * 2 * d
    with pytest.raises(ValueError):
        ScaledDotProductAttention(4)(torch.rand(3, 4, 6))         # 6 is not 3 * 4 * d
    x = torch.rand(2, 3, 12, requires_grad=True)
    assert ScaledDotProductAttention(2)(x) is not x
