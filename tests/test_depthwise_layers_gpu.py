"""Depthwise Conv1d / Conv2d layers reach csrc/depthwise.hip through backend/extensions.py, and nothing else does (bound: see the kernels' test)."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from oracle import vivit_oracle as oracle
from vivit_amd import kernels
from vivit_amd.backend import SqrtGGNExact, backpack, extend
from vivit_amd.backend import extensions as ext

pytestmark = pytest.mark.gpu
EPS, V, N = 2.0 ** -24, 2, 2


def rules_fp64(layer, weight, x, M):
    """``(input rule, weight rule per sample)`` of the conv ``layer`` with ``weight`` (no bias) by fp64 autograd on the CPU."""
    w, x, M = (t.detach().cpu().double() for t in (weight, x, M))
    w.requires_grad_(True)
    xi = x.repeat(V, *[1] * (x.dim() - 1)).requires_grad_(True)
    gin = torch.autograd.grad(layer._conv_forward(xi, w, None), xi, M.flatten(0, 1))[0].view(V, *x.shape)
    gw = [[torch.autograd.grad(layer._conv_forward(x[n:n + 1], w, None), w, M[v, n:n + 1])[0] for n in range(N)] for v in range(V)]
    return gin, torch.stack([torch.stack(g) for g in gw])


DW, OLD = ("dwconv2d_jac_t", "dwconv2d_weight_mjp"), ("conv2d_jac_t", "conv2d_weight_mjp")


@pytest.mark.parametrize("layer,size,forbidden", [(nn.Conv2d(8, 8, 3, padding=1, groups=8, bias=False), (6, 5), OLD),
                                                  (nn.Conv2d(8, 16, (3, 2), stride=2, groups=8, bias=False), (7, 6), OLD),
                                                  (nn.Conv1d(8, 8, 4, padding=3, groups=8, bias=False), (9,), OLD),
                                                  (nn.Conv2d(3, 3, 3, groups=3, bias=False), (5, 5), DW),     # routing left these alone
                                                  (nn.Conv2d(8, 8, 3, groups=2, bias=False), (5, 5), DW)])
def test_layers_take_their_kernels(layer, size, forbidden, monkeypatch):
    """Depthwise layers (groups == in_channels >= 4) must not touch the groups = 1 kernels, the others not the depthwise ones."""
    torch.manual_seed(7)
    layer = layer.cuda()
    x = torch.randn(N, layer.in_channels, *size, device="cuda")
    M = torch.randn(V, *layer(x).shape, device="cuda")
    for name in forbidden:
        monkeypatch.delattr(kernels, name)   # a call of it raises AttributeError
    got = ext._jac_t_mat_prod(layer, M, x), ext._param_factor(layer, "weight", M, x)
    n_terms = (layer.out_channels // layer.groups * int(np.prod(layer.kernel_size)), M[0, 0, 0].numel())
    refs, mags = rules_fp64(layer, layer.weight, x, M), rules_fp64(layer, layer.weight.abs(), x.abs(), M.abs())
    for g, r, mag, n in zip(got, refs, mags, n_terms):
        assert bool(((g.cpu().double() - r).abs() <= (n + 2) * EPS * mag).all())


def test_convnext_stem_ggn_block():
    """V^T V of the depthwise weight's factor is its block of the fp64 GGN (tolerance: tests/test_backend.py::test_vivit_closures)."""
    torch.manual_seed(3)
    model = nn.Sequential(nn.Conv2d(4, 4, 7, padding=3, groups=4), nn.Flatten(), nn.Linear(4 * 6 * 6, 3))
    X, y = torch.rand(3, 4, 6, 6), torch.randint(0, 3, (3,))
    P = model[0].weight.numel()
    block = oracle.dense_ggn(copy.deepcopy(model).double(), X.double(), "ce")[:P, :P]
    model, lossf = extend(model.cuda()), extend(nn.CrossEntropyLoss())
    with backpack(SqrtGGNExact()):
        lossf(model(X.cuda()), y.cuda()).backward()
    Vw = model[0].weight.sqrt_ggn_exact.flatten(2).flatten(0, 1).cpu().double()
    np.testing.assert_allclose((Vw.T @ Vw).numpy(), block.numpy(), rtol=1e-4, atol=1e-5 * block.abs().max().item())
