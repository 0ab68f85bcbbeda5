"""Logit soft-capping (``softcap``, ``SoftCap``) and relative-position bias tables (``bias``, ``alibi_bias``) of the attention modules
in the factor provider, end to end on two small language-model blocks -- host and hip flavours, built as
tests/test_attention_masked_layers.py is, with its sizes and its tolerances.  The factors of the padded batch equal the brute-force
oracle's on the fp64 model and the Gram matrix of the ViViT closures is the Gram matrix of those factors; a batch shorter than the
table's ``max_len`` uses the middle of the table; the caps of the fixtures are felt (the mean of t^2 exceeds 0.05, asserted), so a
rule that dropped the factor 1 - t^2 could not pass.

On the commit before the feature every case of this file fails: the modules take no ``softcap`` and no ``bias`` table, and there is no
``SoftCap`` and no ``alibi_bias``."""
import numpy as np
import pytest
import torch
from torch import nn

import loss_weighted_refs as refs
from helpers import OracleBackend, set_kernel_backend
from oracle import vivit_oracle as oracle
from vivit_amd.backend import (MultiheadSelfAttention, Permute, RotaryEmbedding, ScaledDotProductAttention, SoftCap, SqrtGGNExact,
                               ViViTGGNExact, alibi_bias, backpack, extend)

FLAVOURS = [pytest.param("host", id="host"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
F64 = torch.float64
PAD = -100
VOCAB, E, H, HKV, D, C, T = 7, 8, 4, 2, 2, 3, 5
LENGTHS = (5, 3, 1, 0)          # sample 0 is full, sample 3 is padding from its first position on
N = len(LENGTHS)
ATT_CAP, OUT_CAP = 2.0, 1.5
MAX_LEN = T + 3                 # of the ALiBi table: the batch is shorter


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
    ``gemma``: Embedding -> RMSNorm -> Linear -> RotaryEmbedding -> causal grouped-query attention leaf with ``softcap = 2`` -> Linear
    -> Linear head -> ``SoftCap(1.5)`` -> Permute; ``gemma_window``: the same with ``window = 3`` (Gemma-2's local layers);
    ``bloom``: Embedding -> LayerNorm -> the causal MultiheadSelfAttention container with an ALiBi table for ``MAX_LEN > T`` positions
    -> Linear head -> Permute, no rotary; ``bloom_exact``: the table for exactly ``T`` positions."""
    torch.manual_seed(0)
    if name.startswith("gemma"):
        window = 3 if name == "gemma_window" else None
        body = [nn.RMSNorm(E, eps=1e-5), nn.Linear(E, (H + 2 * HKV) * D), RotaryEmbedding(H, num_kv_heads=HKV),
                ScaledDotProductAttention(H, causal=True, num_kv_heads=HKV, window=window, softcap=ATT_CAP), nn.Linear(E, E),
                nn.Linear(E, C), SoftCap(OUT_CAP)]
    else:
        table = alibi_bias(H, MAX_LEN if name == "bloom" else T)
        body = [nn.LayerNorm(E), MultiheadSelfAttention(E, H, bias=table, causal=True), nn.Linear(E, C)]
    model = nn.Sequential(nn.Embedding(VOCAB, E), *body, Permute(0, 2, 1))
    g = torch.Generator().manual_seed(1)
    for m in model.modules():
        if isinstance(m, nn.Linear):
            for p in m.parameters():
                p.data.copy_(torch.rand(p.shape, generator=g) * 1.2 - 0.5)
        if isinstance(m, (nn.RMSNorm, nn.LayerNorm)):
            m.weight.data.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
    X, y = torch.randint(0, VOCAB, (N, T), generator=g), torch.randint(0, C, (N, T), generator=g)
    for n, L in enumerate(LENGTHS):
        y[n, L:] = PAD
    return model, X, y, nn.CrossEntropyLoss(ignore_index=PAD, reduction="sum")


PROBLEMS = ["gemma", "gemma_window", "bloom"]


def set_lengths(model, lengths):
    """Through the container where there is one (it hands them to its leaf), on the leaf otherwise."""
    owners = [m for m in model if isinstance(m, (MultiheadSelfAttention, ScaledDotProductAttention))]
    assert len(owners) == 1
    owners[0].set_lengths(lengths)


_REFERENCE = {}


def reference(name):
    """fp64, computed once per problem and never written to: the oracle's factors of the padded batch through the fp64 model."""
    if name not in _REFERENCE:
        model, X, y, lossf = make_problem(name)
        ref = nn.Sequential(IdsFromFloat(), *model).double()
        set_lengths(ref, list(LENGTHS))
        Xf = X.double()
        out = ref(Xf).detach()
        S = refs.exact_factor(out, lossf, y).flatten(2)
        _REFERENCE[name] = oracle.sqrt_ggn_factors(ref, Xf, S, None)
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


def factors_on(name, device, subsampling=None, extensions=None, lengths=LENGTHS):
    model, X, y, lossf = make_problem(name)
    model, X, y = model.to(device), X.to(device), y.to(device)
    set_lengths(model, None if lengths is None else list(lengths))
    run_backward(model, X, y, lossf, extensions or [SqrtGGNExact(subsampling=subsampling)])
    return model


def live_pairs():
    """``[N, T, T]`` bool: the pairs (query, key) of live positions with ``j <= i``."""
    t = torch.arange(T)
    live = t[None, :] < torch.tensor(LENGTHS)[:, None]
    return live[:, :, None] & live[:, None, :] & (t[:, None] >= t[None, :])


@pytest.mark.parametrize("problem", ["gemma", "gemma_window"])
def test_the_caps_of_the_fixture_are_felt(problem):
    """The mean of t^2 = tanh^2(z / cap) over the live causal pairs of the attention leaf, and over the live positions of the capped
    final logits, exceeds 0.05 in fp64: 1 - t^2 is far from 1, and a rule without it is far from the reference."""
    model, X, y, lossf = make_problem(problem)
    ref = model.double()
    set_lengths(ref, list(LENGTHS))
    seen = {}
    leaf = [m for m in ref if isinstance(m, ScaledDotProductAttention)][0]
    cap = [m for m in ref if isinstance(m, SoftCap)][0]
    handles = [leaf.register_forward_hook(lambda m, i, o: seen.update(qkv=i[0])), cap.register_forward_hook(lambda m, i, o: seen.update(z=i[0]))]
    ref(X)
    for h in handles:
        h.remove()
    qkv = seen["qkv"]
    q = qkv[..., :H * D].reshape(N, T, HKV, H // HKV, D).permute(0, 2, 3, 1, 4)
    k = qkv[..., H * D:(H + HKV) * D].reshape(N, T, HKV, 1, D).permute(0, 2, 3, 1, 4)
    t2 = torch.tanh((q @ k.transpose(-1, -2)) * leaf.scale_for(D) / ATT_CAP) ** 2                    # [N, Hkv, R, T, T]
    pairs = live_pairs()[:, None, None].expand_as(t2)
    attention_t2 = t2[pairs].mean().item()
    live = torch.tensor([[t < L for t in range(T)] for L in LENGTHS])
    logits_t2 = (torch.tanh(seen["z"] / OUT_CAP) ** 2)[live].mean().item()
    print(f"mean t^2: attention {attention_t2:.3f}, final logits {logits_t2:.3f}")
    assert attention_t2 > 0.05 and logits_t2 > 0.05


@pytest.mark.parametrize("problem", PROBLEMS)
def test_factors_and_gram_matrix(problem, device):
    V_ref = reference(problem)
    model = factors_on(problem, device, extensions=[SqrtGGNExact(), ViViTGGNExact()])
    assert len(V_ref) == len(list(model.parameters()))
    assert all(float(v.abs().max()) > 1e-3 for v in V_ref)
    for p, v in zip(model.parameters(), V_ref):
        close(p.sqrt_ggn_exact, v, rtol=1e-4, atol=1e-6)
        gram = oracle.pairwise_dot(v, start_dim=2, flatten=False)                       # [C T, N, C T, N]
        close(p.vivit_ggn_exact["gram_mat"](), gram, rtol=1e-4, atol=1e-6)
    Vm = torch.cat([p.sqrt_ggn_exact.flatten(2) for p in model.parameters()], 2).cpu()  # [C T, N, P]
    assert bool((Vm[:, LENGTHS.index(0)] == 0).all())


def test_a_rule_without_the_caps_derivative_is_far_from_the_reference():
    """fp64 against fp64: the factors of the same block with the cap's derivative dropped in the attention rule (the scores are still
    capped) miss the reference by far more than the tolerance of the test above."""
    from vivit_amd.backend import extensions

    V_ref = reference("gemma")
    model, X, y, lossf = make_problem("gemma")
    model = model.double()
    set_lengths(model, list(LENGTHS))
    real = extensions._attention_jac_t_torch

    class NoCap:
        def __init__(self, module):
            self._m = module

        def __getattr__(self, name):
            return None if name == "softcap" else getattr(self._m, name)

    extensions._attention_jac_t_torch = lambda module, *a, **k: real(NoCap(module), *a, **k)
    try:
        run_backward(model, X, y, lossf, [SqrtGGNExact()])
    finally:
        extensions._attention_jac_t_torch = real
    first = next(iter(model.parameters()))                                              # the embedding: behind the attention leaf
    err = (first.sqrt_ggn_exact - V_ref[0]).abs()
    assert bool((err > 100 * (1e-4 * V_ref[0].abs() + 1e-6)).any())


def test_a_batch_shorter_than_the_table(device):
    """The ALiBi table for ``MAX_LEN`` positions on a batch of ``T``: the factors of the table for exactly ``T``, byte for byte (the
    middle of the longer table IS the shorter one), and a batch longer than the table is refused by the forward pass."""
    longer, exact = factors_on("bloom", device), factors_on("bloom_exact", device)
    leaf = longer[2][1]
    assert tuple(leaf.bias.shape) == (H, 2 * MAX_LEN - 1) and leaf.bias.device.type == device.type
    assert torch.equal(leaf.bias_for(T).cpu(), alibi_bias(H, T))
    for p, q in zip(longer.parameters(), exact.parameters()):
        assert torch.equal(p.sqrt_ggn_exact, q.sqrt_ggn_exact)
    model, X, y, lossf = make_problem("bloom_exact")
    model = model.to(device)
    with pytest.raises(ValueError, match=f"at most {T}"):
        model(torch.zeros(N, T + 1, dtype=torch.long, device=device))


@pytest.mark.parametrize("subsampling", [[0, 0, 1, 3, 1], [1]], ids=["repeated", "one"])
@pytest.mark.parametrize("problem", ["gemma_window", "bloom"])
def test_subsampling(problem, subsampling, device):
    V_ref = reference(problem)
    model = factors_on(problem, device, subsampling)
    for p, v in zip(model.parameters(), V_ref):
        assert p.sqrt_ggn_exact.shape[1] == len(subsampling)
        close(p.sqrt_ggn_exact, v[:, subsampling], rtol=1e-4, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("problem", ["gemma_window", "bloom"])
def test_the_blocks_run_on_the_hip_kernels(problem, monkeypatch):
    """On the GPU no rule of either block may reach ``torch.autograd.grad`` (the generic input rule), ``torch.einsum`` or
    ``torch.func.vmap``: the attention with a cap or a table is one launch of the HIP kernels, and so is ``SoftCap``."""

    def forbidden(*a, **k):
        raise AssertionError("fell back to the torch rule")

    from vivit_amd import kernels
    calls, kinds = [], []
    real, real_act = kernels.attention_jac_t, kernels.act_jac_t

    def spy(*a, **k):
        calls.append((k.get("softcap"), k.get("bias"), k.get("window")))
        return real(*a, **k)

    def spy_act(M, x, kind, param=0.0):
        kinds.append((kind, param))
        return real_act(M, x, kind, param)

    set_kernel_backend(None)
    dev = torch.device("cuda:0")
    V_ref = reference(problem)
    model, X, y, lossf = make_problem(problem)
    model, X, y = model.to(dev), X.to(dev), y.to(dev)
    set_lengths(model, list(LENGTHS))
    monkeypatch.setattr(torch, "einsum", forbidden)
    monkeypatch.setattr(torch.autograd, "grad", forbidden)
    monkeypatch.setattr(torch.func, "vmap", forbidden)
    monkeypatch.setattr(kernels, "attention_jac_t", spy)
    monkeypatch.setattr(kernels, "act_jac_t", spy_act)
    run_backward(model, X, y, lossf, [SqrtGGNExact()])
    monkeypatch.undo()
    assert len(calls) == 1
    softcap, bias, window = calls[0]
    if problem == "bloom":
        assert softcap is None and window is None and kinds == []
        assert bias.is_cuda and bias.dtype == torch.float32 and bias.is_contiguous() and torch.equal(bias.cpu(), alibi_bias(H, T))
    else:
        assert softcap == ATT_CAP and bias is None and window == 3 and kinds == [("softcap", OUT_CAP)]
    for p, v in zip(model.parameters(), V_ref):
        close(p.sqrt_ggn_exact, v, rtol=1e-4, atol=1e-6)
