"""Padded batches (``set_lengths``) and sliding windows (``window``) of the attention modules in the factor provider, end to end on a
small language-model block -- host and hip flavours, built as tests/test_attention_gqa_layers.py is.  The factors of the padded batch
equal the brute-force oracle's on the fp64 model, their per-sample GGN equals the one of each sequence cut to its length and run
ALONE through a model that knows nothing of lengths (Jacobians and the loss Hessian by autograd in fp64), and the Gram matrix of the
ViViT closures is the Gram matrix of those factors.  Tolerances: those of tests/test_attention_gqa_layers.py for the factors and of
tests/test_loss_positions_layers.py for the Gram matrix, unchanged; the tolerance of the GGN is what the factors' tolerance implies
(written out in ``ggn_close``).

On the commit before the feature every case of this file fails: the modules take no ``window`` and have no ``set_lengths``."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import loss_weighted_refs as refs
from helpers import OracleBackend, set_kernel_backend
from oracle import vivit_oracle as oracle
from vivit_amd.backend import (MultiheadSelfAttention, Permute, RotaryEmbedding, ScaledDotProductAttention, SqrtGGNExact, ViViTGGNExact,
                               backpack, extend)

FLAVOURS = [pytest.param("host", id="host"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
F64 = torch.float64
PAD = -100
VOCAB, E, H, HKV, D, C, T = 7, 8, 4, 2, 2, 3, 5
LENGTHS = (5, 3, 1, 0)          # sample 0 is full, sample 3 is padding from its first position on
N = len(LENGTHS)


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
    """The token ids of a floating input: the brute-force oracle differentiates a model of a floating ``X``."""

    def forward(self, x):
        return x.long()


def make_problem(name):
    """(model, X, y, loss function) on right-padded token ids ``X [N, T]`` with the targets of the padded positions ignored:
    ``decoder``: Embedding -> RMSNorm -> Linear -> RotaryEmbedding -> causal grouped-query attention leaf -> Linear -> Linear head ->
    Permute; ``decoder_window``: the same with ``window = 3``; ``encoder``: Embedding -> RMSNorm -> the MultiheadSelfAttention container
    (not causal, grouped queries) -> Linear head -> Permute; ``encoder_window``: its window is 2."""
    torch.manual_seed(0)
    window = {"decoder": None, "decoder_window": 3, "encoder": None, "encoder_window": 2}[name]
    if name.startswith("decoder"):
        attention = [nn.Linear(E, (H + 2 * HKV) * D), RotaryEmbedding(H, num_kv_heads=HKV),
                     ScaledDotProductAttention(H, causal=True, num_kv_heads=HKV, window=window), nn.Linear(E, E)]
    else:
        attention = [MultiheadSelfAttention(E, H, causal=False, num_kv_heads=HKV, window=window)]
    model = nn.Sequential(nn.Embedding(VOCAB, E), nn.RMSNorm(E, eps=1e-5), *attention, nn.Linear(E, C), Permute(0, 2, 1))
    g = torch.Generator().manual_seed(1)
    for m in model.modules():
        if isinstance(m, nn.Linear):
            for p in m.parameters():
                p.data.copy_(torch.rand(p.shape, generator=g) * 1.2 - 0.5)
        if isinstance(m, nn.RMSNorm):
            m.weight.data.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
    X, y = torch.randint(0, VOCAB, (N, T), generator=g), torch.randint(0, C, (N, T), generator=g)
    for n, L in enumerate(LENGTHS):
        y[n, L:] = PAD
    return model, X, y, nn.CrossEntropyLoss(ignore_index=PAD, reduction="sum")


PROBLEMS = ["decoder", "decoder_window", "encoder", "encoder_window"]


def set_lengths(model, lengths):
    """Through the container where there is one (it hands them to its leaf), on the leaf otherwise."""
    owners = [m for m in model if isinstance(m, (MultiheadSelfAttention, ScaledDotProductAttention))]
    assert len(owners) == 1
    owners[0].set_lengths(lengths)


_REFERENCE = {}


def reference(name):
    """fp64, computed once per problem and never written to: (a) the oracle's factors of the PADDED batch through the model with
    lengths, (b) per sample the GGN of the sequence cut to its length and run alone through the model WITHOUT lengths:
    J^T H J with J and the Hessian H of the summed cross entropy by autograd."""
    if name not in _REFERENCE:
        model, X, y, lossf = make_problem(name)
        ref = nn.Sequential(IdsFromFloat(), *model).double()
        set_lengths(ref, list(LENGTHS))
        Xf = X.double()
        out = ref(Xf).detach()
        S = refs.exact_factor(out, lossf, y).flatten(2)
        V_ref = oracle.sqrt_ggn_factors(ref, Xf, S, None)
        set_lengths(ref, None)
        ggn = []
        for n, L in enumerate(LENGTHS):
            if L == 0:
                ggn.append(None)
                continue
            jac = oracle.per_sample_jacobians(ref, Xf[n:n + 1, :L])                     # [1, C L, *param]
            J = torch.cat([j.reshape(C * L, -1) for j in jac], 1)
            z = ref(Xf[n:n + 1, :L]).detach()
            Hz = torch.autograd.functional.hessian(lambda o: F.cross_entropy(o, y[n:n + 1, :L], reduction="sum"), z).reshape(C * L, C * L)
            ggn.append(J.T @ Hz @ J)
        _REFERENCE[name] = (V_ref, ggn)
    return _REFERENCE[name]


def run_backward(model, X, y, lossf, extensions, hook=None):
    model, lossf = extend(model), extend(lossf)
    model.zero_grad()
    loss = lossf(model(X), y)
    with backpack(*extensions, extension_hook=hook):
        loss.backward()
    return loss


def close(a, b, rtol=1e-4, atol=1e-6):
    np.testing.assert_allclose(a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy(), rtol=rtol, atol=atol)


def ggn_close(Vn, want, rtol=1e-4, atol=1e-6):
    """``Vn [V, P]`` (fp32 factor rows of one sample, each entry within ``rtol |v| + atol`` of the truth: the factors' tolerance) ->
    ``Vn^T Vn`` against ``want``: to first order entry (p, q) is off by at most sum_v (dv_p |v_q| + |v_p| dv_q)."""
    Vn = Vn.double()
    A = Vn.abs()
    tol = 2 * rtol * (A.T @ A) + atol * (A.sum(0)[:, None] + A.sum(0)[None, :]) + 1e-12
    err = (Vn.T @ Vn - want).abs()
    assert bool((err <= tol).all()), f"worst error / tolerance = {(err / tol).max().item():.3g}"


def factors_on(name, device, subsampling=None, extensions=None, lengths=LENGTHS):
    model, X, y, lossf = make_problem(name)
    model, X, y = model.to(device), X.to(device), y.to(device)
    set_lengths(model, None if lengths is None else list(lengths))
    run_backward(model, X, y, lossf, extensions or [SqrtGGNExact(subsampling=subsampling)])
    return model


def test_the_reference_of_the_padded_batch_is_the_reference_of_the_sequences_alone():
    """fp64 against fp64: the two references of this file agree, and a padded position has no factor."""
    for name in PROBLEMS:
        V_ref, ggn = reference(name)
        Vm = torch.cat([v.flatten(2) for v in V_ref], 2)                                # [C T, N, P]
        assert all(float(v.abs().max()) > 1e-3 for v in V_ref)
        for n, L in enumerate(LENGTHS):
            G = Vm[:, n].T @ Vm[:, n]
            if L == 0:
                assert bool((Vm[:, n] == 0).all())
            else:
                assert (G - ggn[n]).abs().max().item() <= 1e-11 * max(1.0, ggn[n].abs().max().item())


@pytest.mark.parametrize("problem", PROBLEMS)
def test_factors_and_gram_matrix_of_a_padded_batch(problem, device):
    V_ref, ggn = reference(problem)
    model = factors_on(problem, device, extensions=[SqrtGGNExact(), ViViTGGNExact()])
    assert len(V_ref) == len(list(model.parameters()))
    for p, v in zip(model.parameters(), V_ref):
        close(p.sqrt_ggn_exact, v, rtol=1e-4, atol=1e-6)
        gram = oracle.pairwise_dot(v, start_dim=2, flatten=False)                       # [C T, N, C T, N]
        close(p.vivit_ggn_exact["gram_mat"](), gram, rtol=1e-4, atol=1e-6)
    Vm = torch.cat([p.sqrt_ggn_exact.flatten(2) for p in model.parameters()], 2).cpu()  # [C T, N, P]
    for n, L in enumerate(LENGTHS):
        if L == 0:
            assert bool((Vm[:, n] == 0).all())
        else:
            ggn_close(Vm[:, n], ggn[n])


@pytest.mark.parametrize("subsampling", [[0, 0, 1, 3, 1], [2, 0, 1, 3], [1]], ids=["repeated", "permuted", "one"])
@pytest.mark.parametrize("problem", ["decoder", "encoder_window"])
def test_subsampling_takes_the_lengths_along(problem, subsampling, device):
    V_ref, _ = reference(problem)
    model = factors_on(problem, device, subsampling)
    for p, v in zip(model.parameters(), V_ref):
        assert p.sqrt_ggn_exact.shape[1] == len(subsampling)
        close(p.sqrt_ggn_exact, v[:, subsampling], rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("problem", ["decoder_window", "encoder"])
def test_resetting_the_lengths_restores_the_unpadded_function(problem, device):
    fresh = factors_on(problem, device, lengths=None)
    model, X, y, lossf = make_problem(problem)
    model, X, y = model.to(device), X.to(device), y.to(device)
    set_lengths(model, list(LENGTHS))
    padded = model(X).detach().clone()
    set_lengths(model, None)
    run_backward(model, X, y, lossf, [SqrtGGNExact()])
    leaf = [m for m in model.modules() if isinstance(m, ScaledDotProductAttention)][0]
    assert leaf.forward_lengths is None
    assert not torch.equal(model(X), padded)
    for p, q in zip(model.parameters(), fresh.parameters()):
        assert torch.equal(p.sqrt_ggn_exact, q.sqrt_ggn_exact)


def test_lengths_hold_until_reset_and_must_match_the_batch(device):
    model, X, y, lossf = make_problem("decoder")
    model, X = model.to(device), X.to(device)
    set_lengths(model, list(LENGTHS))
    a, b = model(X), model(X)                                                           # every forward pass until they are reset
    assert torch.equal(a, b)
    dead = torch.tensor([[t >= L for t in range(T)] for L in LENGTHS])
    leaf = [m for m in model.modules() if isinstance(m, ScaledDotProductAttention)][0]
    assert leaf.forward_lengths.dtype == torch.int32 and leaf.forward_lengths.device.type == device.type
    assert leaf.forward_lengths.tolist() == list(LENGTHS)
    seen = {}
    handle = leaf.register_forward_hook(lambda m, i, o: seen.update(out=o))
    model(X)
    handle.remove()
    assert bool((seen["out"].cpu()[dead] == 0).all())
    with pytest.raises(ValueError, match="4 lengths, the batch has 3"):
        model(X[:3])
    set_lengths(model, torch.tensor(LENGTHS, device=device))                            # a tensor on the device: the same function
    assert torch.equal(model(X), a)
    set_lengths(model, [5, 3])
    with pytest.raises(ValueError, match="2 lengths, the batch has 4"):
        model(X)
    container = MultiheadSelfAttention(E, H, num_kv_heads=HKV)
    container.set_lengths([1, 2])
    assert container[1]._lengths.tolist() == [1, 2] and copy.deepcopy(container)[1]._lengths.tolist() == [1, 2]
    container.set_lengths(None)
    assert container[1]._lengths is None


@pytest.mark.gpu
def test_the_padded_block_runs_on_the_hip_kernels(monkeypatch):
    """On the GPU no rule of the padded, windowed decoder block may reach ``torch.autograd.grad`` (the generic input rule),
    ``torch.einsum`` or ``torch.func.vmap``: the attention with lengths and a window is a launch of the HIP kernels."""

    def forbidden(*a, **k):
        raise AssertionError("fell back to the torch rule")

    from vivit_amd import kernels
    calls = []
    real = kernels.attention_jac_t

    def spy(*a, **k):
        calls.append((k.get("lengths"), k.get("window")))
        return real(*a, **k)

    set_kernel_backend(None)
    dev = torch.device("cuda:0")
    V_ref, _ = reference("decoder_window")
    model, X, y, lossf = make_problem("decoder_window")
    model, X, y = model.to(dev), X.to(dev), y.to(dev)
    set_lengths(model, list(LENGTHS))
    monkeypatch.setattr(torch, "einsum", forbidden)
    monkeypatch.setattr(torch.autograd, "grad", forbidden)
    monkeypatch.setattr(torch.func, "vmap", forbidden)
    monkeypatch.setattr(kernels, "attention_jac_t", spy)
    run_backward(model, X, y, lossf, [SqrtGGNExact()])
    monkeypatch.undo()
    assert len(calls) == 1 and calls[0][1] == 3 and calls[0][0].is_cuda and calls[0][0].tolist() == list(LENGTHS)
    for p, v in zip(model.parameters(), V_ref):
        close(p.sqrt_ggn_exact, v, rtol=1e-4, atol=1e-6)
