"""nn.RMSNorm, the gated product (ProductModule) and rotary position embeddings (RotaryEmbedding) in the factor provider, against the
brute-force autograd oracle, and the Computation classes end to end on models that contain them -- a LLaMA-style decoder block among
them -- host and hip flavours, built as tests/test_norm_layers.py is.  Tolerances: those of tests/test_norm_layers.py and
tests/test_attention_layers.py, unchanged.

On the commit before these rules every case of this file fails at import (no ProductModule / RotaryEmbedding); the problems without
the new modules ("rms_silu_ce", "rms_frozen_ce", "rms_chw_ce") fail there with "no parameter rule for RMSNorm"."""
import math

import numpy as np
import pytest
import torch
from torch import nn

import vivit_amd
from helpers import OracleBackend, constant_damping, set_kernel_backend, top_k_criterion
from oracle import vivit_oracle as oracle
from vivit_amd.backend import (ActiveIdentity, BatchGrad, Parallel, ProductModule, RotaryEmbedding, ScaledDotProductAttention, Slicing,
                               SqrtGGNExact, SqrtGGNMC, backpack, extend)

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
    """Weights of the RMSNorms away from their initial 1 (a rule that forgets gamma must show)."""
    for m in model.modules():
        if isinstance(m, nn.RMSNorm) and m.weight is not None:
            m.weight.data.uniform_(0.5, 1.5)
    return model


def swiglu(E, F_):
    return Parallel(nn.Sequential(nn.Linear(E, F_), nn.SiLU()), nn.Linear(E, F_), merge_module=ProductModule())


class Twice(nn.Module):
    """Feeds one tensor to both inputs of its merge module (a container: the merge module is the leaf)."""

    def __init__(self):
        super().__init__()
        self.merge = ProductModule()

    def forward(self, x):
        return self.merge(x, x)


def make_problem(name):
    torch.manual_seed(0)
    if name == "rms_silu_ce":            # (a)
        model = nn.Sequential(nn.Linear(7, 6), nn.RMSNorm(6, eps=1e-5), nn.SiLU(), nn.Linear(6, 5))
        X, y, lossf, loss = torch.rand(3, 7), torch.randint(0, 5, (3,)), nn.CrossEntropyLoss(), "ce"
    elif name == "rms_swiglu_mse":       # (b): A = 4 rows per sample, eps=None, a gated MLP
        model = nn.Sequential(nn.Linear(5, 3), nn.RMSNorm(3, eps=None), swiglu(3, 4), nn.Linear(4, 2), nn.Flatten())
        X, y, lossf, loss = torch.rand(3, 4, 5), torch.rand(3, 8), nn.MSELoss(), "mse"
    elif name == "rms_frozen_ce":        # (c): no affine parameters, and a frozen weight; eps of the module's own
        frozen = nn.RMSNorm(6, eps=0.3)
        model = nn.Sequential(nn.Linear(7, 6), nn.RMSNorm(6, eps=0.2, elementwise_affine=False), nn.SiLU(), frozen, nn.Linear(6, 4))
        X, y, lossf, loss = torch.rand(3, 7), torch.randint(0, 4, (3,)), nn.CrossEntropyLoss(), "ce"
        reinit(model)
        frozen.weight.requires_grad_(False)
    elif name == "rms_chw_ce":           # (d): normalized_shape with several dimensions
        model = nn.Sequential(nn.Conv2d(2, 3, 2), nn.RMSNorm([3, 3, 4], eps=1e-6), nn.Flatten(), nn.Linear(36, 3))
        X, y, lossf, loss = torch.rand(3, 2, 4, 5), torch.randint(0, 3, (3,)), nn.CrossEntropyLoss(), "ce"
    elif name == "decoder_ce":           # (e): a full decoder block on [N, T, E], T = 5, E = 8, two heads
        E, H = 8, 2
        attention = nn.Sequential(nn.RMSNorm(E, eps=1e-5), nn.Linear(E, 3 * E), RotaryEmbedding(H), ScaledDotProductAttention(H, causal=True),
                                  nn.Linear(E, E))
        mlp = nn.Sequential(nn.RMSNorm(E, eps=1e-5), swiglu(E, 12), nn.Linear(12, E))
        model = nn.Sequential(Parallel(ActiveIdentity(), attention), Parallel(ActiveIdentity(), mlp), nn.RMSNorm(E, eps=1e-5),
                              Slicing((slice(None), -1)), nn.Linear(E, 3))
        X, y, lossf, loss = torch.randn(3, 5, E), torch.randint(0, 3, (3,)), nn.CrossEntropyLoss(), "ce"
        reinit(model)
        model[-1].weight.data.mul_(0.25)   # (as tests/test_embedding_layers.py scales its head: spectra of order one)
    elif name == "square_ce":            # (f): ProductModule fed the same tensor twice
        model = nn.Sequential(nn.Linear(7, 6), Twice(), nn.Linear(6, 4))
        X, y, lossf, loss = torch.rand(3, 7), torch.randint(0, 4, (3,)), nn.CrossEntropyLoss(), "ce"
    return reinit(model), X, y, lossf, loss


PROBLEMS = ["rms_silu_ce", "rms_swiglu_mse", "rms_frozen_ce", "rms_chw_ce", "decoder_ce", "square_ce"]


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


@pytest.mark.parametrize("problem", ["rms_silu_ce", "decoder_ce"])
def test_mc_factors_with_supplied_samples(problem, device):
    model, X, y, lossf, loss = make_problem(problem)
    ref_model = make_problem(problem)[0]
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
    ``torch.func.vmap``: RMSNorm, the gated product, the rotary embedding, the attention and SiLU are launches of the HIP kernels."""

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


@pytest.mark.parametrize("problem", PROBLEMS)
def test_host_rules_do_not_use_autograd(problem, monkeypatch):
    """The torch formulas of non-HIP tensors: RMSNorm, the product and the rotary embedding never reach the generic autograd rule
    there either (activations on host tensors do, as before)."""
    from vivit_amd.backend import extensions

    generic = extensions._generic_jac_t_mat_prod

    def forbidden(module, M, x):
        assert not isinstance(module, (nn.RMSNorm, ProductModule, RotaryEmbedding)), "fell back to the generic autograd rule"
        return generic(module, M, x)

    set_kernel_backend(OracleBackend())
    try:
        model, X, y, lossf, _ = make_problem(problem)
        monkeypatch.setattr(extensions, "_generic_jac_t_mat_prod", forbidden)
        run_backward(model, X, y, lossf, [SqrtGGNExact()])
    finally:
        set_kernel_backend(None)
    assert all(hasattr(p, "sqrt_ggn_exact") for p in trainable(model))


@pytest.mark.parametrize("groups_kind", ["one", "per_parameter"])
@pytest.mark.parametrize("problem", ["rms_silu_ce", "decoder_ce"])
def test_eigvalsh_and_eigh_end_to_end(problem, groups_kind, device):
    """Gram eigenvalues == dense-GGN eigenvalues on the top min(n, P); G e = lambda e; orthonormal -- as
    tests/test_norm_layers.py::test_eigvalsh_and_eigh_end_to_end, with one group and with one group per parameter."""
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
    # (a parameter whose GGN block is below the criterion's floor selects no direction: nothing to compare there)
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


@pytest.mark.parametrize("problem", ["rms_silu_ce", "decoder_ce"])
def test_damped_newton_end_to_end(problem, device):
    """Newton step == the oracle's restatement on autograd factors, as tests/test_norm_layers.py::test_damped_newton_end_to_end."""
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


# ---- the modules themselves -----------------------------------------------------------------------------------------------------
def rotary_fp64(qkv, H, base=10000.0):
    """An independent restatement: element by element, the angle t * base^(-2 j / d) as the module's fp32 table rounds it is NOT
    used -- the angle is computed in fp64 from the fp32 inverse frequency the definition prescribes."""
    N, T, E3 = qkv.shape
    d = E3 // (3 * H)
    out = qkv.double().clone()
    x = qkv.double()
    for t in range(T):
        for which in range(2):
            for h in range(H):
                for j in range(d // 2):
                    a = t * base ** (-2.0 * j / d)
                    i1 = which * H * d + h * d + j
                    i2 = i1 + d // 2
                    out[:, t, i1] = x[:, t, i1] * math.cos(a) - x[:, t, i2] * math.sin(a)
                    out[:, t, i2] = x[:, t, i2] * math.cos(a) + x[:, t, i1] * math.sin(a)
    return out


@pytest.mark.parametrize("H,d,T", [(1, 2, 1), (2, 4, 5), (3, 6, 7)])
def test_rotary_forward(H, d, T):
    qkv = torch.randn(2, T, 3 * H * d, generator=torch.Generator().manual_seed(H + d))
    mod = RotaryEmbedding(H)
    got = mod(qkv)
    ref = rotary_fp64(qkv, H)
    # The module's angles are fp32 by definition: the exponent -2 j / d is rounded (eps, times ln(base) = 9.2 on base^e), powf adds
    # 2 ulp = 4 eps and the product t f one eps: 15 eps relative on an angle of at most T - 1.  cos / sin: 2 ulp = 4 eps; the rotation:
    # 2 eps (|x1 c| + |x2 s|).  In all (15 (T - 1) + 6) eps (|x1| + |x2|), rounded up.
    bound = 2.0 ** -24 * (16 * (T - 1) + 8) * 2 * qkv.abs().max().item()
    assert (got.double() - ref).abs().max().item() <= bound
    E = H * d
    assert torch.equal(got[..., 2 * E:], qkv[..., 2 * E:])                 # v passes through
    assert torch.equal(got[:, 0], qkv[:, 0])                              # position 0: the identity
    cos, sin = mod.tables(T, d, qkv.device, qkv.dtype)
    assert cos.shape == sin.shape == (T, d // 2) and cos.dtype == torch.float32
    assert mod.tables(T, d, qkv.device, qkv.dtype)[0] is cos               # cached: the rule sees the tensors of the forward pass
    got64 = RotaryEmbedding(H)(qkv.double())
    assert got64.dtype == torch.float64 and (got64 - ref).abs().max().item() <= bound   # (fp32 angles, by the definition)


def test_module_errors():
    with pytest.raises(ValueError):
        ProductModule()(torch.zeros(2, 3))
    with pytest.raises(ValueError):
        ProductModule()(torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(2, 3))
    with pytest.raises(ValueError):
        ProductModule()(torch.zeros(2, 3), torch.zeros(2, 1))
    assert torch.equal(ProductModule()(torch.full((2, 3), 2.0), torch.full((2, 3), 3.0)), torch.full((2, 3), 6.0))
    with pytest.raises(ValueError):
        RotaryEmbedding(0)
    with pytest.raises(ValueError):
        RotaryEmbedding(2)(torch.zeros(1, 4, 3 * 2 * 3))      # d = 3 is odd
    with pytest.raises(ValueError):
        RotaryEmbedding(2)(torch.zeros(1, 4, 13))             # not 3 * H * d
    with pytest.raises(ValueError):
        RotaryEmbedding(2)(torch.zeros(4, 12))                # not [N, T, 3 E]
    assert {"ProductModule", "RotaryEmbedding"} <= set(vivit_amd.backend.__all__)
