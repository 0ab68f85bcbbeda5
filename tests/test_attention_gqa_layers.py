"""Grouped-query attention (``num_kv_heads``) in the factor provider, against the brute-force autograd oracle, and the Computation
classes end to end on a LLaMA-style decoder block that uses it -- host and hip flavours, built as tests/test_attention_layers.py and
tests/test_loss_weighted_layers.py are.  Tolerances: theirs, unchanged.

On the commit before the rule every case of this file fails: the modules take no ``num_kv_heads``."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import attention_gqa_refs as gr
import loss_weighted_refs as refs
import vivit_amd
from helpers import OracleBackend, set_kernel_backend
from oracle import vivit_oracle as oracle
from vivit_amd.backend import (ActiveIdentity, BatchGrad, MultiheadSelfAttention, Parallel, Permute, ProductModule, RotaryEmbedding,
                               ScaledDotProductAttention, SqrtGGNExact, backpack, extend)
from vivit_amd.backend.extensions import _jac_t_mat_prod

FLAVOURS = [pytest.param("host", id="host"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
F64 = torch.float64
PAD = -100


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
    """Every weight and bias away from symmetric or trivial values; the RMSNorm weights around 1."""
    g = torch.Generator().manual_seed(1)
    for m in model.modules():
        if isinstance(m, nn.Linear):
            for p in m.parameters():
                p.data.copy_(torch.rand(p.shape, generator=g) * 1.2 - 0.5)
        if isinstance(m, nn.RMSNorm) and m.weight is not None:
            m.weight.data.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
    return model


def swiglu(E, F_):
    return Parallel(nn.Sequential(nn.Linear(E, F_), nn.SiLU()), nn.Linear(E, F_), merge_module=ProductModule())


def make_problem(name):
    """(model, X, y, loss function): (a) the leaf between projections, H = 4, Hkv = 2, d = 2; (b) a LLaMA-style decoder block with
    multi-query attention (H = 4, Hkv = 1, d = 4, T = 5, N = 3) under a per-position cross entropy with right-padded targets; (c) the
    container module with H = 4, Hkv = 2, d = 2."""
    torch.manual_seed(0)
    if name == "sdpa_gqa_ce":
        model = nn.Sequential(nn.Linear(6, 16), ScaledDotProductAttention(4, num_kv_heads=2), nn.Linear(8, 6), nn.Flatten(), nn.Linear(24, 5))
        X, y, lossf = torch.rand(3, 4, 6), torch.randint(0, 5, (3,)), nn.CrossEntropyLoss()
        reinit(model)
    elif name == "decoder_mqa_lm_ce":
        H, Hkv, d = 4, 1, 4
        E = H * d
        attention = nn.Sequential(nn.RMSNorm(E, eps=1e-5), nn.Linear(E, (H + 2 * Hkv) * d), RotaryEmbedding(H, num_kv_heads=Hkv),
                                  ScaledDotProductAttention(H, causal=True, num_kv_heads=Hkv), nn.Linear(E, E))
        mlp = nn.Sequential(nn.RMSNorm(E, eps=1e-5), swiglu(E, 12), nn.Linear(12, E))
        model = nn.Sequential(Parallel(ActiveIdentity(), attention), Parallel(ActiveIdentity(), mlp), nn.RMSNorm(E, eps=1e-5),
                              nn.Linear(E, 3), Permute(0, 2, 1))
        X, y = torch.randn(3, 5, E), torch.randint(0, 3, (3, 5))
        y[1, 3:] = PAD
        y[2, :] = PAD                                                   # sample 1 padded from position 3 on, sample 2 entirely
        lossf = nn.CrossEntropyLoss(ignore_index=PAD)
        for m in model.modules():
            if isinstance(m, nn.RMSNorm):
                m.weight.data.uniform_(0.5, 1.5)
        model[-2].weight.data.mul_(0.25)
    elif name == "mhsa_gqa_mse":
        model = nn.Sequential(MultiheadSelfAttention(8, 4, num_kv_heads=2), nn.Flatten())
        X, y, lossf = torch.rand(3, 4, 8), torch.rand(3, 32), nn.MSELoss()
        reinit(model)
    return model, X, y, lossf


PROBLEMS = ["sdpa_gqa_ce", "decoder_mqa_lm_ce", "mhsa_gqa_mse"]


def reference_factors(name, subsampling=None):
    """The oracle's factors and per-sample gradients of the fp64 model."""
    model, X, y, lossf = make_problem(name)
    model, X = model.double(), X.double()
    y = y.double() if y.is_floating_point() else y
    out = model(X).detach()
    if out.dim() == 2:
        S = oracle.loss_hessian_sqrt_exact(out, "ce" if isinstance(lossf, nn.CrossEntropyLoss) else "mse")
        share = lossf
    else:   # per-position cross entropy with ignored positions: the mean is over the counted positions of the whole batch
        N, C = out.shape[:2]
        S = refs.exact_factor(out, lossf, y).flatten(2)
        norm = float(refs.counted_positions(y, C, lossf.ignore_index).sum())
        share = lambda o, t: N * F.cross_entropy(o, t, ignore_index=lossf.ignore_index, reduction="sum") / norm   # noqa: E731
    return model, X, oracle.sqrt_ggn_factors(model, X, S, subsampling), oracle.batch_grads(model, X, y, share, subsampling)


def run_backward(model, X, y, lossf, extensions, hook=None):
    model, lossf = extend(model), extend(lossf)
    model.zero_grad()
    loss = lossf(model(X), y)
    with backpack(*extensions, extension_hook=hook):
        loss.backward()
    return loss


def close(a, b, rtol=1e-4, atol=1e-6):
    np.testing.assert_allclose(a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy(), rtol=rtol, atol=atol)


def test_the_sample_shares_add_up_to_the_gradient_of_the_loss():
    for name in PROBLEMS:
        model, X, _, g_ref = reference_factors(name)
        _, _, y, lossf = make_problem(name)
        y = y.double() if y.is_floating_point() else y
        grads = torch.autograd.grad(lossf(model(X), y), list(model.parameters()))
        for g, total in zip(g_ref, grads):
            close(g.sum(0), total, rtol=1e-10, atol=1e-13)


# ("permuted" has the batch's length: an output that was not sub-sampled would have the right shape and the wrong rows)
@pytest.mark.parametrize("subsampling", [None, [0, 0, 1, 0, 1], [2, 0, 1]], ids=["full", "repeated", "permuted"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_sqrt_ggn_and_batch_grad_factors(problem, subsampling, device):
    _, _, V_ref, g_ref = reference_factors(problem, subsampling)
    model, X, y, lossf = make_problem(problem)
    assert len(V_ref) == len(g_ref) == len(list(model.parameters()))
    assert all(float(v.abs().max()) > 1e-3 for v in V_ref)
    model, X, y = model.to(device), X.to(device), y.to(device)
    run_backward(model, X, y, lossf, [SqrtGGNExact(subsampling=subsampling), BatchGrad(subsampling=subsampling)])
    for p, v, g in zip(model.parameters(), V_ref, g_ref):
        close(p.sqrt_ggn_exact, v, rtol=1e-4, atol=1e-6)
        close(p.grad_batch, g, rtol=1e-4, atol=1e-7)


def test_eigh_end_to_end_on_the_decoder(device):
    """G e = lambda e and orthonormality against the dense GGN (built from the oracle's factors: the loss is per position)."""
    _, _, V_ref, _ = reference_factors("decoder_mqa_lm_ce")
    Vm = torch.cat([v.flatten(2) for v in V_ref], 2).flatten(0, 1)            # [V N, P]
    ggn = Vm.T @ Vm
    model, X, y, lossf = make_problem("decoder_mqa_lm_ce")
    model, X, y = model.to(device), X.to(device), y.to(device)
    comp = vivit_amd.EighComputation(warn_small_eigvals=0.0)
    crit = lambda evals: [i for i in range(evals.numel()) if evals[i].abs() >= max(1e-4, 1e-3 * float(evals[-1]))]   # noqa: E731
    groups = [{"params": list(model.parameters()), "criterion": crit}]
    run_backward(model, X, y, lossf, [comp.get_extension()], comp.get_extension_hook(groups))
    evals, evecs = comp.get_result(groups[0])
    assert evals.numel() > 0
    E = torch.cat([e.flatten(1) for e in evecs], 1).cpu().double()
    np.testing.assert_allclose((E @ E.T).numpy(), np.eye(E.shape[0]), atol=2e-4)
    np.testing.assert_allclose((E @ ggn).numpy(), (evals.cpu().double()[:, None] * E).numpy(), rtol=1e-3, atol=2e-4)


@pytest.mark.gpu
def test_decoder_block_runs_on_the_hip_kernels(monkeypatch):
    """On the GPU no rule of the grouped-query decoder block may reach ``torch.autograd.grad`` (the generic input rule),
    ``torch.einsum`` or ``torch.func.vmap``: the rotary embedding and the attention are launches of the HIP kernels on the new layout."""

    def forbidden(*a, **k):
        raise AssertionError("fell back to the torch rule")

    set_kernel_backend(None)
    dev = torch.device("cuda:0")
    _, _, V_ref, _ = reference_factors("decoder_mqa_lm_ce")
    model, X, y, lossf = make_problem("decoder_mqa_lm_ce")
    model, X, y = model.to(dev), X.to(dev), y.to(dev)
    monkeypatch.setattr(torch, "einsum", forbidden)
    monkeypatch.setattr(torch.autograd, "grad", forbidden)
    monkeypatch.setattr(torch.func, "vmap", forbidden)
    run_backward(model, X, y, lossf, [SqrtGGNExact()])
    monkeypatch.undo()
    for p, v in zip(model.parameters(), V_ref):
        close(p.sqrt_ggn_exact, v, rtol=1e-4, atol=1e-6)


def test_host_rules_do_not_use_autograd(monkeypatch):
    from vivit_amd.backend import extensions

    generic = extensions._generic_jac_t_mat_prod

    def forbidden(module, M, x):
        assert not isinstance(module, (RotaryEmbedding, ScaledDotProductAttention)), "fell back to the generic autograd rule"
        return generic(module, M, x)

    set_kernel_backend(OracleBackend())
    try:
        model, X, y, lossf = make_problem("decoder_mqa_lm_ce")
        monkeypatch.setattr(extensions, "_generic_jac_t_mat_prod", forbidden)
        run_backward(model, X, y, lossf, [SqrtGGNExact()])
    finally:
        set_kernel_backend(None)
    assert all(hasattr(p, "sqrt_ggn_exact") for p in model.parameters())


def test_head_dimension_above_the_kernel_goes_through_the_generic_rule(device):
    V, N, T, H, Hkv, d = 3, 2, 5, 2, 1, gr.D_MAX + 1
    M, qkv, out, scale = gr.make_case(9, V, N, T, H, Hkv, d)
    module = ScaledDotProductAttention(H, num_kv_heads=Hkv)
    G = _jac_t_mat_prod(module, M.to(device), qkv.to(device))
    ref, _ = gr.rule(M, qkv, out, H, Hkv, scale, False)
    assert tuple(G.shape) == (V, N, T, (H + 2 * Hkv) * d)
    torch.testing.assert_close(G.cpu().double(), ref, rtol=1e-4, atol=1e-6)


def test_output_of_another_batch_is_refused(device):
    torch.manual_seed(2)
    module = ScaledDotProductAttention(4, num_kv_heads=2)
    x = torch.rand(3, 4, 16, device=device)
    module.output = module(x)
    sub = [0, 0, 1, 0, 1]
    M = torch.rand(2, 5, 4, 8, device=device)
    got = _jac_t_mat_prod(module, M, x[sub], sub)
    assert tuple(got.shape) == (2, 5, 4, 16)
    module.output = None                                             # (a module called outside the engine: one forward)
    close(got, _jac_t_mat_prod(module, M, x[sub], sub), rtol=1e-5, atol=1e-7)
    module.output = module(x)
    with pytest.raises(ValueError):
        _jac_t_mat_prod(module, M, x[sub])


def test_constructor_and_shape_validation():
    for make in (lambda **k: ScaledDotProductAttention(4, **k), lambda **k: RotaryEmbedding(4, **k),
                 lambda **k: MultiheadSelfAttention(8, 4, **k)):
        with pytest.raises(ValueError, match=r"num_kv_heads \(Hkv\) must be positive, got 0"):
            make(num_kv_heads=0)
        with pytest.raises(ValueError, match=r"num_kv_heads \(Hkv\) must be positive, got -2"):
            make(num_kv_heads=-2)
        with pytest.raises(ValueError, match=r"H = 4.*Hkv = 3"):
            make(num_kv_heads=3)
        assert make(num_kv_heads=4) is not None and make(num_kv_heads=1) is not None
    for module in (ScaledDotProductAttention(4, num_kv_heads=2), RotaryEmbedding(4, num_kv_heads=2)):
        with pytest.raises(ValueError, match=r"\(H \+ 2 Hkv\) d\], got 2 dimensions"):
            module(torch.rand(4, 16))
        with pytest.raises(ValueError, match=r"last dimension \(12\).*\(4 \+ 2 \* 2\)"):
            module(torch.rand(3, 4, 12))                              # 12 = 3 * 4 * 1 is the multi-head layout, not (4 + 4) d
    with pytest.raises(ValueError, match=r"head dimension \(3\) must be even"):
        RotaryEmbedding(4, num_kv_heads=2)(torch.rand(3, 4, 24))
    x = torch.rand(2, 3, 16, requires_grad=True)
    assert ScaledDotProductAttention(4, num_kv_heads=2)(x).shape == (2, 3, 8)
    mhsa = MultiheadSelfAttention(8, 4, num_kv_heads=2)
    assert tuple(mhsa[0].weight.shape) == (16, 8) and mhsa[1].num_kv_heads == 2 and tuple(mhsa[2].weight.shape) == (8, 8)
    assert MultiheadSelfAttention(8, 4)[1].num_kv_heads is None and tuple(MultiheadSelfAttention(8, 4)[0].weight.shape) == (24, 8)


@pytest.mark.parametrize("causal", [False, True])
def test_forward_expands_k_and_v_as_the_definition_says(causal):
    """Query head h attends to key / value head h // R: the module against torch's own attention on ``repeat_interleave``d copies."""
    H, Hkv, d, N, T = 6, 2, 4, 2, 7
    qkv = torch.randn(N, T, (H + 2 * Hkv) * d, dtype=F64, generator=torch.Generator().manual_seed(4))
    got = ScaledDotProductAttention(H, causal=causal, num_kv_heads=Hkv)(qkv)
    q = qkv[..., :H * d].view(N, T, H, d).transpose(1, 2)
    k = qkv[..., H * d:(H + Hkv) * d].view(N, T, Hkv, d).transpose(1, 2).repeat_interleave(H // Hkv, 1)
    v = qkv[..., (H + Hkv) * d:].view(N, T, Hkv, d).transpose(1, 2).repeat_interleave(H // Hkv, 1)
    ref = F.scaled_dot_product_attention(q, k, v, is_causal=causal).transpose(1, 2).reshape(N, T, H * d)
    assert (got - ref).abs().max().item() <= 1e-12
    # the rotary module rotates the H + Hkv heads of q | k exactly as the multi-head module rotates heads, and passes v through
    rot = RotaryEmbedding(H, num_kv_heads=Hkv)(qkv.float())
    as_mha = RotaryEmbedding(1)(torch.cat((qkv.float()[..., :d], qkv.float()[..., H * d:(H + 1) * d], qkv.float()[..., -d:]), -1))
    assert torch.equal(rot[..., :d], as_mha[..., :d]) and torch.equal(rot[..., H * d:(H + 1) * d], as_mha[..., d:2 * d])
    assert torch.equal(rot[..., (H + Hkv) * d:], qkv.float()[..., (H + Hkv) * d:])


def test_modules_without_num_kv_heads_compute_what_they_did():
    """``num_kv_heads=None``: the forward passes are the formulas of the multi-head modules, byte for byte."""
    g = torch.Generator().manual_seed(6)
    N, T, H, d = 2, 5, 3, 4
    qkv = torch.randn(N, T, 3 * H * d, generator=g)
    for causal in (False, True):
        q, k, v = qkv.view(N, T, 3, H, d).permute(2, 0, 3, 1, 4)
        s = (q @ k.transpose(-1, -2)) * d ** -0.5
        if causal:
            s = s.masked_fill(torch.ones(T, T, dtype=torch.bool).triu(1), float("-inf"))
        want = (s.softmax(-1) @ v).transpose(1, 2).reshape(N, T, H * d)
        assert torch.equal(ScaledDotProductAttention(H, causal=causal)(qkv), want)
    mod = RotaryEmbedding(H)
    half = d // 2
    cos, sin = (t.view(1, T, 1, 1, half) for t in mod.tables(T, d, qkv.device, qkv.dtype))
    x = qkv.view(N, T, 3, H, d)
    x1, x2 = x[:, :, :2, :, :half], x[:, :, :2, :, half:]
    want = torch.cat((torch.cat((x1 * cos - x2 * sin, x2 * cos + x1 * sin), -1), x[:, :, 2:]), 2).reshape(N, T, 3 * H * d)
    assert torch.equal(mod(qkv), want)
    torch.manual_seed(0)
    a = MultiheadSelfAttention(12, 3, causal=True)
    x = torch.randn(N, T, 12, generator=g)
    assert torch.equal(a(x), a[2](ScaledDotProductAttention(3, causal=True)(a[0](x))))
    with pytest.raises(ValueError, match=r"not 3 \* 3 heads"):
        ScaledDotProductAttention(3)(torch.rand(2, 5, 15))               # (the messages of the multi-head layout are unchanged)
