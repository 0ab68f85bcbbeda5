"""A tiny Mamba block from the public modules alone: the factors SqrtGGNExact and BatchGrad attach to the scan's A_log and D and to
the first Linear's weight (through the scan's input rule) on the HIP kernels, against an fp64 CPU run of the same model, which takes
the torch loop and the generic rule.  Tolerance: that of tests/test_llama_layers.py for a chain of layers."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from vivit_amd import kernels
from vivit_amd.backend import (BatchGrad, Pad, Parallel, Permute, ProductModule, SelectiveScan, Slicing, SqrtGGNExact, SumModule, backpack,
                               extend)

pytestmark = pytest.mark.gpu
E, D, S, T, N, C = 8, 16, 4, 2 * kernels.SSCAN_CHUNK + 1, 3, 5
ALL = slice(None)


def mamba_block(head):
    pack = Parallel(Pad((0, D + 2 * S)),                                            # u | 0 | 0 | 0
                    nn.Sequential(nn.Linear(D, D), Pad((D, 2 * S))),                # 0 | dt | 0 | 0
                    nn.Sequential(nn.Linear(D, 2 * S, bias=False), Pad((2 * D, 0))),   # 0 | 0 | B | C
                    merge_module=SumModule())
    ssm = nn.Sequential(Slicing((ALL, ALL, slice(0, D))), Permute(0, 2, 1), nn.Conv1d(D, D, 4, padding=3, groups=D),
                        Slicing((ALL, ALL, slice(0, T))), Permute(0, 2, 1), nn.SiLU(), pack, SelectiveScan(D, S))
    gate = nn.Sequential(Slicing((ALL, ALL, slice(D, 2 * D))), nn.SiLU())
    tail = [Slicing((ALL, -1))] if head == "last" else [Permute(0, 2, 1)]
    return nn.Sequential(nn.Linear(E, 2 * D), Parallel(ssm, gate, merge_module=ProductModule()), nn.Linear(D, C), *tail)


def factors(model, X, y):
    model, lossf = extend(model), extend(nn.CrossEntropyLoss())
    with backpack(SqrtGGNExact(), BatchGrad()):
        lossf(model(X), y).backward()
    scan = next(m for m in model.modules() if isinstance(m, SelectiveScan))
    return [(p.sqrt_ggn_exact, p.grad_batch) for p in (scan.A_log, scan.D, model[0].weight)]


@pytest.mark.parametrize("head", ["last", "all"])
def test_mamba_block_factors_match_fp64(head):
    torch.manual_seed(5)
    model = mamba_block(head)
    X, y = torch.randn(N, T, E), torch.randint(0, C, (N,) if head == "last" else (N, T))
    ref = factors(copy.deepcopy(model).double(), X.double(), y)
    got = factors(model.cuda(), X.cuda(), y.cuda())
    for (v, g), (rv, rg) in zip(got, ref):
        np.testing.assert_allclose(v.cpu().double().numpy(), rv.numpy(), rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(g.cpu().double().numpy(), rg.numpy(), rtol=1e-4, atol=1e-7)
