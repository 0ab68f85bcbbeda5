"""The weighted cross-entropy references of tests/loss_weighted_refs.py against torch itself, and the torch path of
``_loss_hessian_sqrt`` against them.  No GPU.

The references are tied to ``torch.autograd.functional.hessian`` of ``F.cross_entropy`` w.r.t. fp64 logits, not to a restated
formula: ``sum_v S_v S_v^T`` of the exact factor, and ``sum_k p_k S^(k) S^(k)^T`` of the sampled factor with every index set to ``k``
(its expectation over ``idx ~ p``), must both be the Hessian of the mini-batch loss -- for 'mean' and 'sum', with and without class
weights, label smoothing 0 and 0.2, class-index targets (scattered ignored positions, one sample ignored entirely) and probability
targets: 16 combinations, on ``[3, 4, 5]`` and ``[3, 4]``.

On the commit before this capability ``test_the_torch_path_matches_the_references`` fails: the factor never looked at the target."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import loss_weighted_refs as refs
from vivit_amd.backend import extend
from vivit_amd.backend import extensions

F64 = torch.float64
IGNORE = -100
COMBOS = list(itertools.product(["mean", "sum"], [False, True], [0.0, 0.2], ["index", "prob"]))
IDS = [f"{r}-{'w' if w else 'now'}-eps{e}-{k}" for r, w, e, k in COMBOS]
SHAPES = [(3, 4, 5), (3, 4)]


def make_case(shape, weighted, kind, dtype=F64):
    gen = torch.Generator().manual_seed(7)
    N, C, D = shape[0], shape[1], tuple(shape[2:])
    z = torch.randn(*shape, generator=gen, dtype=F64).to(dtype)
    w = (torch.rand(C, generator=gen, dtype=F64) + 0.25).to(dtype) if weighted else None
    if kind == "prob":
        t = torch.softmax(torch.randn(*shape, generator=gen, dtype=F64), 1).to(dtype)
    else:
        t = torch.randint(0, C, (N,) + D, generator=gen)
        if D:
            t[0, 1], t[2, 3], t[2, 0] = IGNORE, IGNORE, IGNORE                 # scattered
        t[1] = IGNORE                                                          # one sample ignored entirely
    return z, t, w


def torch_hessian(z, t, w, reduction, eps):
    def f(x):
        return F.cross_entropy(x, t, weight=w, ignore_index=IGNORE, reduction=reduction, label_smoothing=eps)

    return torch.autograd.functional.hessian(f, z.clone()).reshape(z.numel(), z.numel())


@pytest.mark.parametrize("shape", SHAPES, ids=["positions", "flat"])
@pytest.mark.parametrize("reduction,weighted,eps,kind", COMBOS, ids=IDS)
def test_the_exact_reference_factorises_the_autograd_hessian(reduction, weighted, eps, kind, shape):
    z, t, w = make_case(shape, weighted, kind)
    H = torch_hessian(z, t, w, reduction, eps)
    omega = refs.position_weights(t, shape[1], w, IGNORE, eps, reduction)
    S = refs.ce_exact_w(z, omega).flatten(2)                                   # [V, N, C L]
    G = torch.zeros_like(H).reshape(shape[0], S.shape[2], shape[0], S.shape[2])
    for n in range(shape[0]):                                                  # (the loss couples no two samples)
        G[n, :, n, :] = S[:, n].T @ S[:, n]
    np.testing.assert_allclose(G.reshape(H.shape).numpy(), H.numpy(), rtol=1e-12, atol=1e-15)
    if kind == "index":
        assert float(omega[1].abs().max()) == 0.0 and bool((S[:, 1] == 0).all())


@pytest.mark.parametrize("shape", SHAPES, ids=["positions", "flat"])
@pytest.mark.parametrize("reduction,weighted,eps,kind", COMBOS, ids=IDS)
def test_the_sampled_reference_has_the_autograd_hessian_as_its_expectation(reduction, weighted, eps, kind, shape):
    z, t, w = make_case(shape, weighted, kind)
    N, C, D = shape[0], shape[1], tuple(shape[2:])
    H = torch_hessian(z, t, w, reduction, eps)
    omega = refs.position_weights(t, C, w, IGNORE, eps, reduction)
    p = torch.softmax(z, 1)
    # per position: sum_k p_k s_k s_k^T over the classes of that position, zero between positions
    L = z[0, 0].numel()
    Gv = torch.zeros(N, C, L, N, C, L, dtype=F64)
    for k in range(C):
        Sk = refs.ce_sampled_w(z, torch.full((1, N) + D, k), omega)[0].reshape(N, C, L)   # every index is k
        pk = p.reshape(N, C, L)[:, k]                                          # [N, L]
        for n in range(N):
            for l in range(L):
                Gv[n, :, l, n, :, l] += pk[n, l] * torch.outer(Sk[n, :, l], Sk[n, :, l])
    np.testing.assert_allclose(Gv.reshape(H.shape).numpy(), H.numpy(), rtol=1e-12, atol=1e-15)


def test_samples_scale_with_their_number():
    z, t, w = make_case((3, 4, 5), True, "index")
    omega = refs.position_weights(t, 4, w, IGNORE, 0.2, "mean")
    idx = torch.randint(0, 4, (3, 3, 5), generator=torch.Generator().manual_seed(1))
    S3, S1 = refs.ce_sampled_w(z, idx, omega), refs.ce_sampled_w(z, idx[:1], omega)
    np.testing.assert_allclose((S3[0] * 3 ** 0.5).numpy(), S1[0].numpy(), rtol=1e-14, atol=0)


def test_edge_decisions_of_the_weights():
    """Everything ignored: zeros (torch's own loss is NaN).  An out-of-range target that is not ignore_index: weight 0, and it takes no
    part in the normaliser.  A negative weight: NaN under the square root at its positions only."""
    C = 4
    assert float(refs.position_weights(torch.full((2, 3), IGNORE), C).abs().max()) == 0.0
    t = torch.tensor([[0, 7, 1], [-3, 2, IGNORE]])
    om = refs.position_weights(t, C)
    assert om.tolist() == [[1 / 3, 0.0, 1 / 3], [0.0, 1 / 3, 0.0]]
    w = torch.tensor([1.0, -2.0, 4.0, 1.0], dtype=F64)
    s = refs.target_scales(t, C, w, mean=False)
    assert bool(torch.isnan(s[0, 2])) and s[0, 0] == 1.0 and s[1, 1] == 2.0 and s[0, 1] == 0.0
    z = torch.randn(2, C, 3, dtype=F64)
    z[0, :, 1] = float("nan")                                                  # garbage under an uncounted position
    S = refs.ce_exact_w(z, om)
    assert bool(torch.isfinite(S).all()) and bool((S[:, 0, :, 1] == 0).all())


# ---- the torch path of the factor provider ------------------------------------------------------------------------------------------
def recorded_loss(z, t, w, reduction, eps):
    lossf = extend(nn.CrossEntropyLoss(weight=w, ignore_index=IGNORE, reduction=reduction, label_smoothing=eps))
    lossf(z.clone().requires_grad_(True), t)
    return lossf


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=["positions", "flat"])
@pytest.mark.parametrize("reduction,weighted,eps,kind", COMBOS, ids=IDS)
def test_the_torch_path_matches_the_references(reduction, weighted, eps, kind, shape, dtype):
    z, t, w = make_case(shape, weighted, kind, dtype)
    N, C, D = shape[0], shape[1], tuple(shape[2:])
    lossf = recorded_loss(z, t, w, reduction, eps)
    tol = dict(rtol=1e-12, atol=1e-15) if dtype == F64 else dict(rtol=1e-5, atol=1e-7)
    omega = refs.position_weights(t, C, w, IGNORE, eps, reduction)
    S = extensions._loss_hessian_sqrt(lossf, "exact", 1, None)
    assert S.dtype == dtype
    np.testing.assert_allclose(S.double().numpy(), refs.ce_exact_w(z, omega).numpy(), **tol)
    idx = torch.randint(0, C, (3, N) + D, generator=torch.Generator().manual_seed(2))
    samples = idx if D else F.one_hot(idx, C).to(dtype)                        # ([N, C] takes one-hots [M, N, C])
    Smc = extensions._loss_hessian_sqrt(lossf, "sampling", 3, samples)
    np.testing.assert_allclose(Smc.double().numpy(), refs.ce_sampled_w(z, idx, omega).numpy(), **tol)


@pytest.mark.parametrize("shape", SHAPES, ids=["positions", "flat"])
def test_garbage_under_ignored_positions_does_not_reach_the_factor(shape):
    z, t, w = make_case(shape, True, "index", torch.float32)
    z[1] = float("nan")                                                        # the sample that is ignored entirely
    lossf = recorded_loss(z, t, w, "mean", 0.0)
    S = extensions._loss_hessian_sqrt(lossf, "exact", 1, None)
    assert bool(torch.isfinite(S).all()) and bool((S[:, 1] == 0).all()) and float(S[:, 0].abs().max()) > 0


def test_a_loss_without_a_recorded_target_is_the_unweighted_factor():
    z, t, w = make_case((3, 4, 5), True, "index", torch.float32)
    lossf = recorded_loss(z, t, w, "mean", 0.2)
    del lossf.input1
    S = extensions._loss_hessian_sqrt(lossf, "exact", 1, None)
    import loss_positions_refs as base

    np.testing.assert_allclose(S.double().numpy(), base.ce_exact_vec(z, 1.0 / 15 ** 0.5).numpy(), rtol=1e-5, atol=1e-7)
