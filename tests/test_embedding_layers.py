"""nn.Embedding in the factor provider, against the brute-force autograd oracle, and the Computation classes end to end on models that
start from token ids -- host and hip flavours, built as tests/test_attention_layers.py is.  The model input is integer: the oracle
(which allocates its Jacobians in the dtype of the input) is given the ids as floats and a first module that turns them back."""
import numpy as np
import pytest
import torch
from torch import nn

import vivit_amd
from helpers import OracleBackend, set_kernel_backend
from oracle import vivit_oracle as oracle
from vivit_amd.backend import (
    ActiveIdentity,
    BatchGrad,
    MultiheadSelfAttention,
    Parallel,
    Slicing,
    SqrtGGNExact,
    SqrtGGNMC,
    ViViTGGNExact,
    backpack,
    extend,
)

FLAVOURS = [pytest.param("host", id="host"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
SUBSAMPLINGS = pytest.mark.parametrize("subsampling", [None, [0, 0, 1, 0, 1], [2, 0, 1]], ids=["full", "repeated", "permuted"])


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
    """Float token ids -> int64 (the oracle's side only)."""

    def forward(self, x):
        return x.round().long()


def reinit(model):
    """Every weight and bias away from symmetric or trivial values (as tests/test_attention_layers.py)."""
    g = torch.Generator().manual_seed(1)
    for p in model.parameters():
        p.data.copy_(torch.rand(p.shape, generator=g) * 1.2 - 0.5)
    for m in model.modules():
        if isinstance(m, nn.LayerNorm):
            m.weight.data.add_(1.0)
    return model


def make_problem(name):
    torch.manual_seed(0)
    if name == "flat_ce":            # (a): token 1 twice in sample 0, token 5 twice in sample 2, token 4 in samples 0 and 1
        model = nn.Sequential(nn.Embedding(11, 6), nn.Flatten(), nn.Linear(24, 5))
        X = torch.tensor([[1, 4, 1, 7], [4, 2, 9, 10], [0, 3, 5, 5]])
        y, lossf, loss = torch.randint(0, 5, (3,)), nn.CrossEntropyLoss(), "ce"
    elif name == "encoder_mse":      # (b): the encoder block of tests/test_attention_layers.py on embedded tokens, 0 = padding
        E = 8
        model = nn.Sequential(
            nn.Embedding(9, E, padding_idx=0),
            Parallel(ActiveIdentity(), nn.Sequential(nn.LayerNorm(E), MultiheadSelfAttention(E, 2, causal=True))),
            Parallel(ActiveIdentity(), nn.Sequential(nn.LayerNorm(E), nn.Linear(E, 12), nn.GELU(), nn.Linear(12, E))),
            Slicing((slice(None), 0)), nn.Linear(E, 3))
        # (the class token reads position 0 only -- the attention is causal: sample 1 starts with padding, samples 0 and 2 share token 3)
        X = torch.tensor([[3, 1, 0, 0, 2], [0, 5, 7, 0, 1], [3, 2, 3, 4, 0]])
        y, lossf, loss = torch.rand(3, 3), nn.MSELoss(), "mse"
    elif name == "encoder_full":     # (c): (b) without the causal mask -- the class token hears every position, so the factor at the
        E = 8                        # embedding output is dense: token 3 twice in sample 2, padding inside samples 0 and 1
        model = nn.Sequential(
            nn.Embedding(9, E, padding_idx=0),
            Parallel(ActiveIdentity(), nn.Sequential(nn.LayerNorm(E), MultiheadSelfAttention(E, 2, causal=False))),
            Parallel(ActiveIdentity(), nn.Sequential(nn.LayerNorm(E), nn.Linear(E, 12), nn.GELU(), nn.Linear(12, E))),
            Slicing((slice(None), 0)), nn.Linear(E, 3))
        X = torch.tensor([[3, 1, 0, 0, 2], [0, 5, 7, 0, 1], [3, 2, 3, 4, 0]])
        y, lossf, loss = torch.rand(3, 3), nn.MSELoss(), "mse"
    model = reinit(model)
    if name in ("encoder_mse", "encoder_full"):
        # LayerNorm on rows of standard deviation 0.35 amplifies the Jacobian: with the head as drawn the largest GGN eigenvalue is 49,
        # and the absolute tolerances taken over from tests/test_norm_layers.py are those of fp32 spectra of order one
        model[-1].weight.data.mul_(0.25)
    return model, X, y, lossf, loss


def make_reference(name, double=False):
    """The same model behind :class:`IdsFromFloat`, and its float input."""
    model, X, y, lossf, loss = make_problem(name)
    ref = nn.Sequential(IdsFromFloat(), *model)
    return (ref.double(), X.double()) if double else (ref, X.float())


PROBLEMS = ["flat_ce", "encoder_mse", "encoder_full"]


def run_backward(model, X, y, lossf, extensions, hook=None):
    model, lossf = extend(model), extend(lossf)
    model.zero_grad()
    loss = lossf(model(X), y)
    with backpack(*extensions, extension_hook=hook):
        loss.backward()
    return loss


def close(a, b, rtol=1e-4, atol=1e-6):
    np.testing.assert_allclose(a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy(), rtol=rtol, atol=atol)


@SUBSAMPLINGS
@pytest.mark.parametrize("problem", PROBLEMS)
def test_sqrt_ggn_and_batch_grad_factors(problem, subsampling, device):
    model, X, y, lossf, loss = make_problem(problem)
    ref_model, Xf = make_reference(problem)
    S = oracle.loss_hessian_sqrt_exact(ref_model(Xf).detach(), loss)
    V_ref = oracle.sqrt_ggn_factors(ref_model, Xf, S, subsampling)
    g_ref = oracle.batch_grads(ref_model, Xf, y, lossf, subsampling)
    assert len(V_ref) == len(g_ref) == len(list(model.parameters()))
    assert float(V_ref[0].abs().max()) > 1e-3                         # the embedding weight's factor is not trivially zero

    model, X, y = model.to(device), X.to(device), y.to(device)
    run_backward(model, X, y, lossf, [SqrtGGNExact(subsampling=subsampling), BatchGrad(subsampling=subsampling)])
    for p, v, g in zip(model.parameters(), V_ref, g_ref):
        close(p.sqrt_ggn_exact, v, rtol=1e-4, atol=1e-6)
        close(p.grad_batch, g, rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize("problem", PROBLEMS)
def test_mc_factors_with_supplied_samples(problem, device):
    """Supplied samples: one-hot class draws for the cross-entropy, standard-normal draws for the squared error."""
    model, X, y, lossf, loss = make_problem(problem)
    ref_model, Xf = make_reference(problem)
    out = ref_model(Xf).detach()
    gen = torch.Generator().manual_seed(1)
    if loss == "ce":
        idx = torch.multinomial(out.softmax(1), 3, replacement=True, generator=gen)
        samples = torch.nn.functional.one_hot(idx.t(), out.shape[1]).to(out.dtype)
        S = oracle.loss_hessian_sqrt_mc(out, samples)
    else:
        samples = torch.randn(3, *out.shape, generator=gen)
        S = oracle.loss_hessian_sqrt_mc_mse(samples)
    V_ref = oracle.sqrt_ggn_factors(ref_model, Xf, S)
    assert float(V_ref[0].abs().max()) > 1e-3
    model, X, y = model.to(device), X.to(device), y.to(device)
    run_backward(model, X, y, lossf, [SqrtGGNMC(mc_samples=3, samples=samples)])
    for p, v in zip(model.parameters(), V_ref):
        close(p.sqrt_ggn_mc, v, rtol=1e-4, atol=1e-6)


@SUBSAMPLINGS
@pytest.mark.parametrize("problem", PROBLEMS)
def test_vivit_closures(problem, subsampling, device):
    """gram_mat, V_mat_prod, V_t_mat_prod and factor() of the embedding weight against the same quantities of the oracle's factor."""
    model, X, y, lossf, loss = make_problem(problem)
    ref_model, Xf = make_reference(problem)
    S = oracle.loss_hessian_sqrt_exact(ref_model(Xf).detach(), loss)
    V_ref = oracle.sqrt_ggn_factors(ref_model, Xf, S, subsampling)[0]                  # [C, N, W, D]
    model, X, y = model.to(device), X.to(device), y.to(device)
    run_backward(model, X, y, lossf, [ViViTGGNExact(subsampling=subsampling)])
    closures = next(model.parameters()).vivit_ggn_exact
    assert set(closures) == {"V_mat_prod", "V_t_mat_prod", "gram_mat", "factor", "shape_cn", "dp_add"}
    C, N = closures["shape_cn"]
    assert (C, N) == tuple(V_ref.shape[:2])
    gram_ref = oracle.pairwise_dot(V_ref, start_dim=2, flatten=False)
    gram = closures["gram_mat"]()
    close(gram, gram_ref, rtol=1e-4, atol=1e-7)
    prior = torch.rand(C, N, C, N, generator=torch.Generator().manual_seed(2))
    acc = prior.clone().to(device)
    assert closures["gram_mat"](out=acc, beta=1.0).data_ptr() == acc.data_ptr()
    close(acc, gram_ref + prior, rtol=1e-4, atol=1e-6)
    g = torch.Generator().manual_seed(3)
    mat = torch.randn(4, C, N, generator=g)
    close(closures["V_mat_prod"](mat.to(device)), oracle.Vmp(V_ref, mat, 2), rtol=1e-4, atol=1e-6)
    mat = torch.randn(4, *V_ref.shape[2:], generator=g)
    close(closures["V_t_mat_prod"](mat.to(device)), oracle.mVp(V_ref, mat, 2), rtol=1e-4, atol=1e-6)
    close(closures["factor"](), V_ref, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("groups_kind", ["one", "embedding"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_eigvalsh_and_eigh_end_to_end(problem, groups_kind, device):
    """Gram eigenvalues == dense-GGN eigenvalues, G e = lambda e and orthonormality, as tests/test_norm_layers.py does: one group of
    all parameters, and the embedding weight as a group of its own."""
    model, X, y, lossf, loss = make_problem(problem)
    ref_model, Xd = make_reference(problem, double=True)
    model, X, y = model.to(device), X.to(device), y.to(device)
    params = list(model.parameters())
    ggn = oracle.dense_ggn(ref_model, Xd, loss)
    idx = list(range(len(params))) if groups_kind == "one" else [0]
    numel = sum(params[i].numel() for i in idx)      # (the embedding weight is the first parameter: a leading block in either case)
    block = ggn[:numel][:, :numel]
    ref_w = torch.linalg.eigvalsh(block)
    assert float(ref_w[-1]) >= 1e-4

    comp = vivit_amd.EigvalshComputation()
    group = {"params": [params[i] for i in idx]}
    run_backward(model, X, y, lossf, [comp.get_extension()], comp.get_extension_hook([group]))
    w = comp.get_result(group).cpu().double()
    k = min(len(w), len(ref_w))
    np.testing.assert_allclose(w[-k:].numpy(), ref_w[-k:].numpy(), rtol=1e-4, atol=5e-6)

    comp = vivit_amd.EighComputation(warn_small_eigvals=0.0)
    crit = lambda evals: [i for i in range(evals.numel()) if evals[i].abs() >= max(1e-4, 1e-3 * float(evals[-1]))]   # noqa: E731
    group = {"params": [params[i] for i in idx], "criterion": crit}
    run_backward(model, X, y, lossf, [comp.get_extension()], comp.get_extension_hook([group]))
    evals, evecs = comp.get_result(group)
    assert evals.numel() > 0
    E = torch.cat([e.flatten(1) for e in evecs], 1).cpu().double()
    np.testing.assert_allclose((E @ E.T).numpy(), np.eye(E.shape[0]), atol=2e-4)
    np.testing.assert_allclose((E @ block).numpy(), (evals.cpu().double()[:, None] * E).numpy(), rtol=1e-3, atol=2e-4)


@pytest.mark.gpu
def test_embedded_encoder_runs_on_the_hip_kernels(monkeypatch):
    """On the GPU neither the factors nor the closures' Gram matrix of problem (b) may reach ``torch.einsum``, ``torch.autograd.grad``,
    ``torch.func.vmap`` or ``Tensor.index_add_``: the embedding rule is launches of the kernels of csrc/embedding.hip."""

    def forbidden(*a, **k):
        raise AssertionError("fell back to the torch rule")

    set_kernel_backend(None)
    dev = torch.device("cuda:0")
    model, X, y, lossf, loss = make_problem("encoder_mse")
    ref_model, Xf = make_reference("encoder_mse")
    S = oracle.loss_hessian_sqrt_exact(ref_model(Xf).detach(), loss)
    V_ref = oracle.sqrt_ggn_factors(ref_model, Xf, S, None)
    gram_ref = oracle.pairwise_dot(V_ref[0], start_dim=2, flatten=False)
    model, X, y = model.to(dev), X.to(dev), y.to(dev)
    monkeypatch.setattr(torch, "einsum", forbidden)
    monkeypatch.setattr(torch.autograd, "grad", forbidden)
    monkeypatch.setattr(torch.func, "vmap", forbidden)
    monkeypatch.setattr(torch.Tensor, "index_add_", forbidden)
    run_backward(model, X, y, lossf, [SqrtGGNExact(), ViViTGGNExact()])
    gram = next(model.parameters()).vivit_ggn_exact["gram_mat"]()
    monkeypatch.undo()
    for p, v in zip(model.parameters(), V_ref):
        close(p.sqrt_ggn_exact, v, rtol=1e-4, atol=1e-6)
    close(gram, gram_ref, rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize("option", [dict(max_norm=1.0), dict(scale_grad_by_freq=True)], ids=["max_norm", "scale_grad_by_freq"])
def test_unsupported_options_are_named(option, device):
    model = nn.Sequential(nn.Embedding(11, 6, **option), nn.Flatten(), nn.Linear(24, 5)).to(device)
    _, X, y, lossf, _ = make_problem("flat_ce")
    for ext in (SqrtGGNExact(), BatchGrad(), ViViTGGNExact()):
        with pytest.raises(NotImplementedError, match=next(iter(option))):
            run_backward(model, X.to(device), y.to(device), lossf, [ext])


def test_sparse_gradients_are_accepted(device):
    """``sparse=True`` changes the layout of autograd's own weight gradient, nothing the factors are made of."""
    model, X, y, lossf, loss = make_problem("flat_ce")
    sparse = nn.Sequential(nn.Embedding(11, 6, sparse=True), nn.Flatten(), nn.Linear(24, 5))
    sparse.load_state_dict(model.state_dict())
    ref_model, Xf = make_reference("flat_ce")
    S = oracle.loss_hessian_sqrt_exact(ref_model(Xf).detach(), loss)
    V_ref = oracle.sqrt_ggn_factors(ref_model, Xf, S, None)
    sparse, X, y = sparse.to(device), X.to(device), y.to(device)
    run_backward(sparse, X, y, lossf, [SqrtGGNExact()])
    for p, v in zip(sparse.parameters(), V_ref):
        close(p.sqrt_ggn_exact, v, rtol=1e-4, atol=1e-6)
