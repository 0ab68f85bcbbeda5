"""Learned relative-position bias tables (``learn_bias``, ``bias_index``, ``relative_position_buckets``) of the attention modules in
the factor provider, end to end on a two-layer encoder of ``MultiheadSelfAttention(learn_attention_bias=True)`` with a per-position
cross-entropy head -- once with a plain table for more positions than the batch has, once with T5's buckets, ``scale = 1`` and a
right-padded batch --, on the host in fp64 and, marked ``gpu``, in fp32 on the device.  The table's factor has the table's shape
behind ``[V, N]`` and equals the brute-force oracle's (autograd's Jacobian) and so does its Gram matrix; the per-sample gradients sum
to ``.grad``; the Gram matrix with the table differs from the one of the same model with a frozen table by exactly the table's block;
sub-sampling repeats rows; a module with ``learn_bias=False`` is the module built without the new arguments, byte for byte.

On the commit before the feature every test of this file fails: the modules take no ``learn_attention_bias``."""
import numpy as np
import pytest
import torch
from torch import nn

import loss_weighted_refs as refs
from helpers import OracleBackend, set_kernel_backend
from oracle import vivit_oracle as oracle
from vivit_amd.backend import (BatchGrad, MultiheadSelfAttention, Permute, ScaledDotProductAttention, SqrtGGNExact, ViViTGGNExact, backpack,
                               extend, relative_position_buckets)

FLAVOURS = [pytest.param("host", id="host"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
F64 = torch.float64
PAD = -100
E, H, C, T, MAX_LEN, BUCKETS = 8, 4, 3, 5, 8, 8
LENGTHS = {"plain": None, "t5": (5, 3, 1, 0)}   # t5: sample 0 is full, sample 3 is padding from its first position on
N = 4
PROBLEMS = ["plain", "t5"]


@pytest.fixture(params=FLAVOURS)
def flavour(request):
    """(device, dtype, rtol, atol): fp64 on the host, fp32 on the device (the tolerances of tests/test_attention_scoremod_layers.py)."""
    if request.param == "host":
        set_kernel_backend(OracleBackend())
        yield torch.device("cpu"), F64, 1e-9, 1e-12
        set_kernel_backend(None)
    else:
        set_kernel_backend(None)
        yield torch.device("cuda:0"), torch.float32, 1e-4, 1e-6


def make_problem(name, learn=True, explicit=True):
    """(model, X, y, loss function): ``MultiheadSelfAttention`` twice, a Linear head and ``Permute`` on ``X [N, T, E]``.  ``plain``: a
    table ``[H, 2 MAX_LEN - 1]`` per layer (the second layer causal); ``t5``: a table ``[H, 8]`` per layer read through
    ``relative_position_buckets(MAX_LEN, 8, 16)`` (bidirectional, the second layer causal and unidirectional), ``scale = 1`` and a
    right-padded batch whose padded targets are ignored.  ``learn=False``: the same tables, frozen; ``explicit=False``: the modules
    are built without the new arguments."""
    g = torch.Generator().manual_seed(3)
    layers = []
    for causal in (False, True):
        kw = {} if not explicit else dict(learn_attention_bias=learn)
        if name == "t5":
            table = torch.randn(H, BUCKETS, generator=g)
            kw["attention_bias_index"] = relative_position_buckets(MAX_LEN, BUCKETS, 16, bidirectional=not causal)
        else:
            table = torch.randn(H, 2 * MAX_LEN - 1, generator=g)
        layer = MultiheadSelfAttention(E, H, causal=causal, attention_bias=table, **kw)
        if name == "t5":
            layer[1].scale = 1.0
        layers.append(layer)
    model = nn.Sequential(*layers, nn.Linear(E, C), Permute(0, 2, 1))
    for m in model.modules():
        if isinstance(m, nn.Linear):
            for p in m.parameters():
                p.data.copy_(torch.rand(p.shape, generator=g) * 1.2 - 0.5)
    X, y = torch.randn(N, T, E, generator=g), torch.randint(0, C, (N, T), generator=g)
    if LENGTHS[name] is not None:
        for n, L in enumerate(LENGTHS[name]):
            y[n, L:] = PAD
    return model, X, y, nn.CrossEntropyLoss(ignore_index=PAD, reduction="sum")


def set_lengths(model, name):
    for m in model:
        if isinstance(m, MultiheadSelfAttention):
            m.set_lengths(None if LENGTHS[name] is None else list(LENGTHS[name]))


def tables(model):
    return [m.bias for m in model.modules() if isinstance(m, ScaledDotProductAttention)]


_REFERENCE = {}


def reference(name):
    """fp64, computed once per problem and never written to: the oracle's factors (autograd's Jacobian of the fp64 model behind the
    exact square root of the loss Hessian), one per parameter in the order of ``model.parameters()``."""
    if name not in _REFERENCE:
        model, X, y, lossf = make_problem(name)
        ref = model.double()
        set_lengths(ref, name)
        Xd = X.double()
        S = refs.exact_factor(ref(Xd).detach(), lossf, y).flatten(2)
        _REFERENCE[name] = oracle.sqrt_ggn_factors(ref, Xd, S, None)
    return _REFERENCE[name]


def run(name, flavour, extensions, **kw):
    device, dtype, _, _ = flavour
    model, X, y, lossf = make_problem(name, **kw)
    model, X, y = model.to(device=device, dtype=dtype), X.to(device=device, dtype=dtype), y.to(device)
    set_lengths(model, name)
    model, lossf = extend(model), extend(lossf)
    model.zero_grad()
    loss = lossf(model(X), y)
    with backpack(*extensions):
        loss.backward()
    return model


def close(a, b, flavour):
    np.testing.assert_allclose(a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy(), rtol=flavour[2], atol=flavour[3])


@pytest.mark.parametrize("problem", PROBLEMS)
def test_the_table_is_a_parameter_with_the_buffers_keys(problem):
    learned, frozen = make_problem(problem)[0], make_problem(problem, learn=False)[0]
    assert list(learned.state_dict()) == list(frozen.state_dict())
    R = BUCKETS if problem == "t5" else 2 * MAX_LEN - 1
    for t in tables(learned):
        assert isinstance(t, nn.Parameter) and t.requires_grad and tuple(t.shape) == (H, R)
    for t in tables(frozen):
        assert not isinstance(t, nn.Parameter) and not t.requires_grad
    assert len(list(learned.parameters())) == len(list(frozen.parameters())) + 2
    leaf = learned[0][1]
    assert tuple(leaf.bias_for(T).shape) == (H, 2 * T - 1)
    if problem == "t5":
        assert "0.1.bias_index" in learned.state_dict() and leaf.bias_index.dtype == torch.int64
        assert torch.equal(leaf.bias_for(T), leaf.bias[:, relative_position_buckets(T, BUCKETS, 16)])
    else:
        assert leaf.bias_for(T).data_ptr() == leaf.bias[:, MAX_LEN - T:].data_ptr()      # without an index: the view it was


@pytest.mark.parametrize("problem", PROBLEMS)
def test_factors_and_gram_matrix(problem, flavour):
    V_ref = reference(problem)
    model = run(problem, flavour, [SqrtGGNExact(), ViViTGGNExact()])
    params = list(model.parameters())
    assert len(V_ref) == len(params)
    R = BUCKETS if problem == "t5" else 2 * MAX_LEN - 1
    seen = 0
    for p, v in zip(params, V_ref):
        if any(p is t for t in tables(model)):
            seen += 1
            assert tuple(p.sqrt_ggn_exact.shape) == (C * T, N, H, R) and float(v.abs().max()) > 1e-3
        close(p.sqrt_ggn_exact, v, flavour)
        close(p.vivit_ggn_exact["gram_mat"](), oracle.pairwise_dot(v, start_dim=2, flatten=False), flavour)
    assert seen == 2
    if LENGTHS[problem] is not None:
        dead = LENGTHS[problem].index(0)
        assert all(bool((p.sqrt_ggn_exact[:, dead] == 0).all()) for p in params)


@pytest.mark.parametrize("problem", PROBLEMS)
def test_per_sample_gradients_sum_to_the_gradient(problem, flavour):
    model = run(problem, flavour, [BatchGrad()])
    for t in tables(model):
        assert tuple(t.grad_batch.shape) == (N, *t.shape) and float(t.grad.abs().max()) > 1e-3
    for p in model.parameters():
        close(p.grad_batch.sum(0), p.grad, flavour)


@pytest.mark.parametrize("problem", PROBLEMS)
def test_the_gram_matrix_gains_exactly_the_tables_block(problem, flavour):
    learned, frozen = (run(problem, flavour, [SqrtGGNExact(), ViViTGGNExact()], learn=learn) for learn in (True, False))
    own = tables(learned)
    others = [p for p in learned.parameters() if not any(p is t for t in own)]
    assert len(others) == len(list(frozen.parameters()))
    for p, q in zip(others, frozen.parameters()):
        assert torch.equal(p.sqrt_ggn_exact, q.sqrt_ggn_exact)
    total = lambda ps: sum(p.vivit_ggn_exact["gram_mat"]().double() for p in ps)   # noqa: E731
    block = total(own)
    assert float(block.abs().max()) > 1e-6
    close(total(learned.parameters()) - total(frozen.parameters()), block, flavour)


@pytest.mark.parametrize("problem", PROBLEMS)
def test_subsampling_repeats_rows(problem, flavour):
    sub = [2, 0, 2]
    V_ref = reference(problem)
    model = run(problem, flavour, [SqrtGGNExact(subsampling=sub)])
    for p, v in zip(model.parameters(), V_ref):
        assert p.sqrt_ggn_exact.shape[1] == len(sub)
        close(p.sqrt_ggn_exact, v[:, sub], flavour)
        assert torch.equal(p.sqrt_ggn_exact[:, 0], p.sqrt_ggn_exact[:, 2])


def test_a_frozen_table_is_the_module_without_the_new_arguments(flavour):
    """(the plain table: one read through buckets cannot be built without ``bias_index``)"""
    new, old = (run("plain", flavour, [SqrtGGNExact()], learn=False, explicit=explicit) for explicit in (True, False))
    assert len(list(new.parameters())) == len(list(old.parameters()))
    for p, q in zip(new.parameters(), old.parameters()):
        assert torch.equal(p.sqrt_ggn_exact, q.sqrt_ggn_exact)
    assert list(new.state_dict()) == list(old.state_dict())


@pytest.mark.gpu
@pytest.mark.parametrize("problem", PROBLEMS)
def test_the_table_runs_on_the_hip_kernel(problem, monkeypatch):
    """On the GPU the table's factor is one call of ``kernels.attention_bias_factor`` per layer, never autograd or the torch formula."""
    from vivit_amd import kernels
    from vivit_amd.backend import extensions

    def forbidden(*a, **k):
        raise AssertionError("fell back to the torch rule")

    calls = []
    real = kernels.attention_bias_factor

    def spy(*a, **k):
        calls.append((a[6], k["index"], k["width"]))
        return real(*a, **k)

    monkeypatch.setattr(torch.autograd, "grad", forbidden)
    monkeypatch.setattr(extensions, "_attention_bias_factor_torch", forbidden)
    monkeypatch.setattr(kernels, "attention_bias_factor", spy)
    set_kernel_backend(None)
    model = run(problem, (torch.device("cuda:0"), torch.float32, 1e-4, 1e-6), [SqrtGGNExact()])
    monkeypatch.undo()
    assert len(calls) == 2
    for (bias, index, width), leaf in zip(reversed(calls), [m for m in model.modules() if isinstance(m, ScaledDotProductAttention)]):
        assert bias.is_cuda and bias.dtype == torch.float32 and tuple(bias.shape) == (H, 2 * T - 1) and not bias.requires_grad
        assert torch.equal(bias, leaf.bias_for(T).detach()) and width == leaf.bias.shape[1] and tuple(index.shape) == (2 * T - 1,)


def test_constructor_errors():
    table, index = torch.zeros(H, 2 * MAX_LEN - 1), relative_position_buckets(MAX_LEN, BUCKETS, 16)
    small = torch.zeros(H, BUCKETS)
    with pytest.raises(ValueError, match="learn_bias=True needs a bias"):
        ScaledDotProductAttention(H, learn_bias=True)
    with pytest.raises(ValueError, match="bias_index indexes a bias table"):
        ScaledDotProductAttention(H, bias_index=index)
    for bad in (index.float(), index.bool(), index[:-1], index.view(1, -1), [0, 1, 2], index - 1):
        with pytest.raises(ValueError, match="bias_index must"):
            ScaledDotProductAttention(H, bias=small, bias_index=bad)
    with pytest.raises(ValueError, match="bias_index reaches entry 7"):
        ScaledDotProductAttention(H, bias=small[:, :7], bias_index=index)
    with pytest.raises(ValueError, match="bias must be a floating-point tensor"):
        ScaledDotProductAttention(H, bias=torch.zeros(H + 1, BUCKETS), bias_index=index)
    with pytest.raises(ValueError, match="bias must be a floating-point tensor"):
        ScaledDotProductAttention(H, bias=torch.zeros(H, 8), learn_bias=True)       # without an index the width must be odd
    with pytest.raises(ValueError, match="bias must be finite"):
        ScaledDotProductAttention(H, bias=torch.full((H, BUCKETS), float("nan")), bias_index=index, learn_bias=True)
    ScaledDotProductAttention(H, bias=torch.zeros(H, 8), bias_index=index)          # with one the table may have any width > max(index)
    with pytest.raises(ValueError, match="learn_bias=True needs a bias"):
        MultiheadSelfAttention(E, H, learn_attention_bias=True)
    leaf = ScaledDotProductAttention(H, bias=table, learn_bias=True)
    with pytest.raises(ValueError, match=f"at most {MAX_LEN}"):
        leaf(torch.zeros(1, MAX_LEN + 1, 3 * E))
    with pytest.raises(ValueError, match="max_len must be positive"):
        relative_position_buckets(0)
