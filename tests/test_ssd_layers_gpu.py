"""Linear -> SelectiveScanSSD -> Linear from the public modules: the factors SqrtGGNExact and BatchGrad attach to the scan's A_log, D,
dt_bias and to the first Linear's weight (through the scan's input rule) on the HIP kernels, and the module's own forward and
backward pass, against fp64 CPU runs through ``scan_loop``.  Tolerance: tests/ssd_refs.bound, with the largest |reference| in the
place of the majorant (a chain of layers has no per-element majorant)."""
import copy

import pytest
import torch
from torch import nn

import ssd_refs as refs
from vivit_amd import kernels
from vivit_amd.backend import BatchGrad, SelectiveScanSSD, Slicing, SqrtGGNExact, backpack, extend

pytestmark = pytest.mark.gpu
E, H, P, S, G, T, N, C = 6, 4, 8, 16, 2, kernels.SSD_CHUNK + 3, 2, 5
WIDTH = H * P + H + 2 * G * S


def stack(d_state=S):
    torch.manual_seed(3)
    model = nn.Sequential(nn.Linear(E, H * P + H + 2 * G * d_state), SelectiveScanSSD(H, P, d_state, G), nn.Linear(H * P, C),
                          Slicing((slice(None), -1)))
    with torch.no_grad():
        model[1].dt_bias.copy_(0.3 * torch.randn(H))
    return model


def close(got, ref, x):
    tol = refs.bound(ref.abs().max(), x, torch.zeros(H), torch.zeros(H), H, P, S, G)
    assert got.shape == ref.shape and float((got.cpu().double() - ref).abs().max()) <= float(tol)


def factors(model, X, y):
    model, lossf = extend(model), extend(nn.MSELoss())
    with backpack(SqrtGGNExact(), BatchGrad()):
        lossf(model(X), y).backward()
    return [f for p in (model[1].A_log, model[1].D, model[1].dt_bias, model[0].weight) for f in (p.sqrt_ggn_exact, p.grad_batch)]


def test_stack_factors_match_fp64_loop():
    model, X, y = stack(), torch.randn(N, T, E), torch.randn(N, C)
    ref = factors(copy.deepcopy(model).double(), X.double(), y.double())
    x = model[0](X).detach()
    for got, want in zip(factors(model.cuda(), X.cuda(), y.cuda()), ref):
        close(got, want, x)


@pytest.mark.parametrize("d_state", [S, 129])   # 129: beyond the kernel, the module runs its loop without a word
def test_module_forward_and_backward_match_the_loop(d_state):
    scan = stack(d_state)[1]
    x = torch.randn(N, T, H * P + H + 2 * G * d_state, requires_grad=True)
    ref = copy.deepcopy(scan).double()
    xr = x.detach().double().requires_grad_()
    ref.scan_loop(xr).square().sum().backward()
    dev, xd = scan.cuda(), x.detach().cuda().requires_grad_()
    out = dev(xd)
    out.square().sum().backward()
    close(out.detach(), ref.scan_loop(xr).detach(), x.detach()[..., :WIDTH])
    for got, want in [(xd.grad, xr.grad)] + [(getattr(dev, k).grad, getattr(ref, k).grad) for k in ("A_log", "D", "dt_bias")]:
        close(got, want, x.detach()[..., :WIDTH])
