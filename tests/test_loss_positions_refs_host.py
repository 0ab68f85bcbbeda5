"""The fp64 references of tests/loss_positions_refs.py against PyTorch itself (no GPU): the factor's outer products sum to the Hessian
of the real ``nn.CrossEntropyLoss`` / ``nn.MSELoss`` on ``[N, C, *D]`` w.r.t. one sample's output, for both reductions -- which pins the
``1 / (N L)`` and ``2 / (N C L)`` normalisations independently of the code under test."""
import math

import numpy as np
import pytest
import torch
from torch import nn

import loss_positions_refs as refs

F64 = torch.float64
SHAPES = [(2, 4, (3,)), (2, 3, (2, 2))]


def problem(N, C, D, loss, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = torch.randn(N, C, *D, generator=g, dtype=F64)
    y = torch.randint(0, C, (N, *D), generator=g) if loss == "ce" else torch.randn(N, C, *D, generator=g, dtype=F64)
    return out, y


def sample_hessian(lossf, out, y, n):
    """Hessian of the mini-batch loss w.r.t. out[n], [C L, C L] (flattened over (c, l))."""
    def f(o):
        return lossf(torch.cat((out[:n], o.unsqueeze(0), out[n + 1:])), y)

    H = torch.autograd.functional.hessian(f, out[n].clone())
    k = out[n].numel()
    return H.reshape(k, k)


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("loss", ["ce", "mse"])
@pytest.mark.parametrize("N,C,D", SHAPES)
def test_exact_factor_squares_to_the_hessian_of_the_real_loss(N, C, D, loss, reduction):
    out, y = problem(N, C, D, loss)
    lossf = (nn.CrossEntropyLoss if loss == "ce" else nn.MSELoss)(reduction=reduction)
    S = refs.exact_factor(out, loss, reduction)
    assert S.shape == (C * math.prod(D), N, C, *D) and S.dtype == F64
    for n in range(N):
        Sn = S[:, n].flatten(1)                                   # [V, C L]
        np.testing.assert_allclose((Sn.T @ Sn).numpy(), sample_hessian(lossf, out, y, n).numpy(), rtol=1e-9)


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("N,C,D", SHAPES)
def test_sampled_ce_factor_averages_to_the_exact_hessian(N, C, D, reduction):
    """With every class index enumerated (slice m draws class m at every position) and weighted by its probability, the sampled
    factor's outer products give each position's block of the Hessian exactly: sum_m p_m (p - e_m)(p - e_m)^T = diag(p) - p p^T."""
    out, y = problem(N, C, D, "ce", seed=1)
    L = math.prod(D)
    lossf = nn.CrossEntropyLoss(reduction=reduction)
    norm = refs.norm_of("ce", reduction, N, C, L)
    idx = torch.arange(C).view(C, 1, *([1] * len(D))).expand(C, N, *D)
    S = refs.ce_sampled(out, idx, 1.0 / math.sqrt(norm)).reshape(C, N, C, L)
    p = out.softmax(1).reshape(N, C, L)
    for n in range(N):
        H = sample_hessian(lossf, out, y, n).reshape(C, L, C, L)
        for l in range(L):
            est = torch.einsum("m,mc,md->cd", p[n, :, l], S[:, n, :, l], S[:, n, :, l])
            np.testing.assert_allclose(est.numpy(), H[:, l, :, l].numpy(), rtol=1e-9)


def same(a, b):
    """Equal values and equal NaN masks, exactly."""
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.isnan() == b.isnan()).all()) and torch.equal(a.nan_to_num(nan=-7.0),
                                                                                                               b.nan_to_num(nan=-7.0))


def edge_outputs(out, kind):
    out = out.clone()
    z = out.view(out.shape[0], out.shape[1], -1)                  # [N, C, L], the same memory
    if kind == "minus_inf_class":
        z[:, 1, :] = float("-inf")
    elif kind == "nan":
        z[1, 2, 0] = float("nan")
    elif kind == "plus_inf":
        z[0, 0, -1] = float("inf")
    elif kind == "all_minus_inf":
        z[1, :, 1] = float("-inf")
    return out


@pytest.mark.parametrize("kind", ["finite", "minus_inf_class", "nan", "plus_inf", "all_minus_inf"])
@pytest.mark.parametrize("dtype", [torch.float32, F64])
@pytest.mark.parametrize("N,C,D", SHAPES)
def test_vectorised_references_equal_the_loops(N, C, D, dtype, kind):
    """``ce_sampled_vec`` / ``ce_exact_vec`` (what the tests at 10^5 to 10^7 positions compare with) give the values of the loops
    bit for bit, out-of-range indices included; on non-finite logits both follow torch: a NaN, a +inf or nothing but -inf poisons its
    position and no other, and the structural zeros of the exact factor stay 0.0."""
    out = edge_outputs(problem(N, C, D, "ce", seed=3)[0].to(dtype), kind)
    idx = torch.randint(0, C, (3, N, *D), generator=torch.Generator().manual_seed(5), dtype=torch.int32)
    idx.view(-1)[[0, 5, 7, 11]] = torch.tensor([-1, C, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32)
    assert same(refs.ce_sampled_vec(out, idx, 0.5), refs.ce_sampled(out, idx, 0.5))
    assert same(refs.ce_sampled_vec(out, idx.long(), 0.5), refs.ce_sampled(out, idx, 0.5))
    E = refs.ce_exact_vec(out, 0.25)
    assert same(E, refs.ce_exact(out, 0.25))
    L = math.prod(D)
    poisoned = out.reshape(N, C, L).softmax(1).isnan().any(1)                                   # [N, L], torch's own verdict
    assert bool(poisoned.any()) == (kind in ("nan", "plus_inf", "all_minus_inf")) and int(poisoned.sum()) <= 1
    assert torch.equal(refs.ce_sampled_vec(out, idx, 0.5).reshape(3, N, C, L).isnan(), poisoned.view(1, N, 1, L).expand(3, N, C, L))
    Ex = E.reshape(C, L, N, C, L)
    off = ~torch.eye(L, dtype=torch.bool)
    assert bool((Ex.permute(1, 4, 0, 2, 3)[off] == 0.0).all())
    diag = Ex.permute(1, 4, 0, 2, 3)[~off]                                                      # [l, c', n, c]
    assert torch.equal(diag.isnan(), poisoned.t().reshape(L, 1, N, 1).expand(L, C, N, C))


def test_sampled_references_follow_their_formulas():
    out, _ = problem(2, 4, (3,), "ce", seed=2)
    idx = torch.tensor([[[0, 3, 1], [2, 2, 0]]])
    S = refs.ce_sampled(out, idx, 0.5)
    onehot = torch.nn.functional.one_hot(idx, 4).movedim(-1, 2).to(F64)
    np.testing.assert_allclose(S.numpy(), ((out.softmax(1).unsqueeze(0) - onehot) * 0.5).numpy(), rtol=1e-12)
    bad = idx.clone()
    bad[0, 1, 2] = 4                                              # outside [0, C): matches no class
    Sb = refs.ce_sampled(out, bad, 0.5)
    np.testing.assert_allclose(Sb[0, 1, :, 2].numpy(), (out.softmax(1)[1, :, 2] * 0.5).numpy(), rtol=1e-12)
    eps = torch.randn(3, 2, 4, 3, dtype=F64)
    assert torch.equal(refs.mse_sampled(eps, 0.25), eps * 0.25)
