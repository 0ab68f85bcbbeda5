"""kernels.dwconv2d_jac_t / dwconv2d_weight_mjp against fp64 autograd of F.conv2d(groups=C) on the CPU (weight rule: per sample) under
|got - ref| <= (n + 2) 2^-24 sum|terms| (tests/conv_family_refs.py), sum|terms| = the rule on |operands|, n = mult KH KW resp. OH OW."""
import functools

import pytest
import torch
import torch.nn.functional as F

from vivit_amd import _lib, kernels

pytestmark = pytest.mark.gpu
F64, EPS = torch.float64, 2.0 ** -24
# rows of the weight rule's strip for 3 x 3, padding 1, W = OW = 4 (dw_weight_plan: SR OW + (SR + 2) XC <= budget, XC = 6)
STRIP = (kernels.DWCONV_LDS_FLOATS - kernels.DWCONV_RED_FLOATS - 2 * 6) // (4 + 6)
CASES = {   # id -> C, mult, kernel, stride, padding, dilation, plane, (V, N)
    "plain": (4, 1, (3, 3), (1, 1), (1, 1), (1, 1), (5, 5), (2, 2)),
    "mult2-per-axis": (5, 2, (3, 2), (2, 3), (1, 0), (1, 1), (7, 6), (2, 2)),
    "taps-in-padding": (4, 1, (3, 3), (1, 1), (3, 3), (2, 2), (1, 1), (2, 2)),
    "stride-beyond-kernel": (4, 1, (2, 2), (3, 3), (0, 0), (1, 1), (7, 7), (2, 2)),
    "convnext-9x11": (6, 1, (7, 7), (1, 1), (3, 3), (1, 1), (9, 11), (2, 2)),
    "conv1d-T=DWCONV_ROW_TILE+3": (8, 1, (1, 4), (1, 1), (0, 3), (1, 1), (1, kernels.DWCONV_ROW_TILE + 3), (2, 2)),
    "input-tile+1-row": (4, 1, (3, 3), (1, 1), (1, 1), (1, 1), (kernels.DWCONV_LANES + 1, 4), (2, 2)),        # W = 4: one group, LANES rows per tile
    "weight-strip+1-row": (4, 1, (3, 3), (1, 1), (1, 1), (1, 1), (STRIP + 1, 4), (2, 2)),
    "33000-planes": (132, 1, (2, 2), (1, 1), (0, 0), (1, 1), (2, 2), (1, 250)),               # weight rule: 8250 work items
    "conv1d-2050-tiles": (205, 1, (1, 4), (1, 1), (0, 3), (1, 1), (1, kernels.DWCONV_ROW_TILE + 3), (1, 5)),  # input rule: past DWCONV_GRID_CAP
    "128-taps": (4, 1, (8, 16), (1, 1), (0, 0), (1, 1), (8, 16), (2, 2)),
}


@functools.lru_cache(maxsize=None)
def problem(name):
    """CPU operands ``(M, W, x)`` and, per rule, ``(fp64 reference, bound)``; computed once, not to be modified."""
    C, mult, k, s, p, d, hw, (V, N) = CASES[name]
    gen = torch.Generator().manual_seed(len(name))
    W, x = torch.randn(C * mult, 1, *k, generator=gen), torch.randn(N, C, *hw, generator=gen)
    conv = functools.partial(F.conv2d, bias=None, stride=s, padding=p, dilation=d, groups=C)
    M = torch.randn(V, *conv(x, W).shape, generator=gen)

    def input_rule(M, W):
        xi = torch.zeros(V * N, C, *hw, dtype=F64, requires_grad=True)
        return torch.autograd.grad(conv(xi, W.to(F64)), xi, M.to(F64).flatten(0, 1))[0].view(V, N, C, *hw)

    def weight_rule(M, x):
        w = torch.zeros(W.shape, dtype=F64, requires_grad=True)
        return torch.stack([torch.stack([torch.autograd.grad(conv(x[n:n + 1].to(F64), w), w, M[v, n:n + 1].to(F64))[0] for n in range(N)])
                            for v in range(V)])

    return (M, W, x), {"input": (input_rule(M, W), (mult * k[0] * k[1] + 2) * EPS * input_rule(M.abs(), W.abs())),
                       "weight": (weight_rule(M, x), (M.shape[3] * M.shape[4] + 2) * EPS * weight_rule(M.abs(), x.abs()))}


def run(name, rule):
    C, mult, k, s, p, d, hw, _ = CASES[name]
    M, W, x = (t.cuda() for t in problem(name)[0])
    if rule == "input":
        return kernels.dwconv2d_jac_t(M, W, hw, s, p, d, mult)
    return kernels.dwconv2d_weight_mjp(M, x, k, s, p, d)


@pytest.mark.parametrize("rule", ["input", "weight"])
@pytest.mark.parametrize("name", list(CASES))
def test_rule_matches_fp64_autograd(name, rule):
    ref, bound = problem(name)[1][rule]
    got = run(name, rule).cpu()
    assert got.shape == ref.shape and bool(((got.to(F64) - ref).abs() <= bound).all())
    assert not torch.signbit(got[bound == 0]).any()   # an element without terms (no window reads it) is +0
    assert name != "convnext-9x11" or torch.equal(run(name, rule).cpu(), got)   # the same bytes on every run


def test_129_taps_are_refused():
    M, W = torch.randn(1, 1, 4, 1, 1).cuda(), torch.randn(4, 1, 3, 43).cuda()
    for call in (lambda: kernels.dwconv2d_jac_t(M, W, (3, 43), (1, 1), (0, 0), (1, 1)),
                 lambda: kernels.dwconv2d_weight_mjp(M, W.view(1, 4, 3, 43), (3, 43), (1, 1), (0, 0), (1, 1))):
        with pytest.raises(_lib.VivitHipError, match="status -4"):   # VIVIT_E_UNSUPPORTED
            call()
