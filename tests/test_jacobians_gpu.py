"""The native layer rules of the factor back-propagation (csrc/jacobians.hip, csrc/factors.hip) one by one against plain
torch autograd of the layer itself -- the definition BackPACK's derivative classes implement for the reference
(vivit/extensions/secondorder/vivit/__init__.py:84-118, base.py:19,41,84-92) -- at shapes of the BASELINE networks and at
awkward ones (strides, paddings, dilation, ragged channel counts), plus the packed-triangle kernels of the multi-GPU
all-reduce.  fp32; tolerances are those of a length-L fp32 sum."""
import math

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import epilogue_refs as R
from oracle import vivit_oracle as oracle

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def jac_t_by_autograd(module, x, M):
    """[V, N, *out] -> [V, N, *in]: vector-Jacobian products of ``module`` at ``x`` for every slice of ``M``."""
    x = x.detach().requires_grad_(True)
    y = module(x)
    return torch.stack([torch.autograd.grad(y, x, grad_outputs=M[v], retain_graph=True)[0] for v in range(M.shape[0])])


def close(a, b, rtol=1e-5, atol=1e-6):
    torch.testing.assert_close(a, b, rtol=rtol, atol=atol)


@pytest.mark.parametrize("kind,module", [("relu", nn.ReLU()), ("sigmoid", nn.Sigmoid()), ("tanh", nn.Tanh()),
                                         ("leaky_relu", nn.LeakyReLU(0.1)), ("logsigmoid", nn.LogSigmoid()),
                                         ("elu", nn.ELU(0.7)), ("selu", nn.SELU())])
def test_activation_rules(kind, module):
    from vivit_amd import kernels

    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(37, 5, 11, generator=g, device=DEV) * 2
    M = torch.randn(3, *x.shape, generator=g, device=DEV)
    param = {"leaky_relu": 0.1, "elu": 0.7}.get(kind, 0.0)
    close(kernels.act_jac_t(M, x, kind, param), jac_t_by_autograd(module, x, M), rtol=2e-5, atol=1e-6)


@pytest.mark.parametrize("shape,k,s,p", [((64, 6, 28, 28), 2, 2, 0), ((9, 5, 13, 11), 3, 2, 1), ((4, 3, 8, 8), 3, 1, 1),
                                         ((3, 2, 7, 9), (2, 3), (1, 2), (1, 0))] + R.POOL_EDGE_GEOMS)
def test_pooling_rules(shape, k, s, p):
    from vivit_amd import kernels
    from vivit_amd.backend.extensions import _pair

    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(*shape, generator=g, device=DEV)
    x[0, 0, :3, :3] = 1.5   # ties inside a window: the first maximum in scan order must take the gradient (as torch)
    for mod in (nn.MaxPool2d(k, s, p), nn.AvgPool2d(k, s, p)):
        y = mod(x)
        M = torch.randn(2, *y.shape, generator=g, device=DEV)
        ref = jac_t_by_autograd(mod, x, M)
        if isinstance(mod, nn.MaxPool2d):
            got = kernels.maxpool2d_jac_t(M, x, _pair(k), _pair(s), _pair(p))
        else:
            got = kernels.avgpool2d_jac_t(M, x.shape[2:], _pair(k), _pair(s), _pair(p))
        close(got, ref)


@pytest.mark.parametrize("cin,cout,hw,k,s,p,d", [(6, 16, (14, 14), 5, 1, 0, 1),      # LeNet conv2
                                                 (16, 32, (32, 32), 3, 2, 1, 1),     # ResNet-32 down-sampling block
                                                 (64, 64, (8, 8), 3, 1, 1, 1),       # ResNet-32 last stage
                                                 (5, 7, (9, 11), (2, 3), (2, 1), (1, 2), (2, 1)),   # ragged everything
                                                 (19, 3, (6, 6), 3, 1, 0, 1),        # more than one group of 16 input channels
                                                 # filter slices beyond the scalar input rule's LDS budget (Cout KH KW > 1024): the
                                                 # matrix-pipe input rule -- one chunk with split contraction, ragged channels and
                                                 # positions, stride 2 (inserted zeros), chunks of output channels
                                                 (40, 128, (8, 8), 3, 1, 1, 1),
                                                 (37, 150, (7, 9), 3, 2, 1, 1),
                                                 (16, 520, (20, 20), 3, 1, 1, 1),
                                                 (8, 72, (12, 12), 5, 1, 2, 1)])
def test_conv2d_rules(cin, cout, hw, k, s, p, d):
    from vivit_amd import kernels

    g = torch.Generator(device=DEV).manual_seed(2)
    N, Vd = 5, 3
    conv = nn.Conv2d(cin, cout, k, stride=s, padding=p, dilation=d, bias=True).to(DEV)
    x = torch.randn(N, cin, *hw, generator=g, device=DEV)
    y = conv(x)
    M = torch.randn(Vd, *y.shape, generator=g, device=DEV)
    # input rule = transposed convolution
    got = kernels.conv2d_jac_t(M, conv.weight.detach(), x.shape[2:], conv.stride, conv.padding, conv.dilation)
    close(got, jac_t_by_autograd(conv, x, M), rtol=1e-4, atol=1e-5)
    # weight rule: per-sample, per-slice gradient of <M[v, n], conv(x[n])> w.r.t. the weight
    gotw = kernels.conv2d_weight_mjp(M, x, conv.kernel_size, conv.stride, conv.padding, conv.dilation)
    ref = torch.empty_like(gotw)
    for v in range(Vd):
        for n in range(N):
            xn = x[n:n + 1]
            ref[v, n] = torch.autograd.grad(F.conv2d(xn, conv.weight, None, conv.stride, conv.padding, conv.dilation),
                                            conv.weight, grad_outputs=M[v, n:n + 1])[0]
    L = y.shape[2] * y.shape[3]
    close(gotw, ref, rtol=1e-4, atol=1e-5 * math.sqrt(L))
    # bias rule: sum over the output positions
    close(kernels.row_dot(M.reshape(-1, L)).view(Vd, N, cout), M.flatten(3).sum(3), rtol=1e-5, atol=1e-5 * math.sqrt(L))


@pytest.mark.parametrize("cin,cout,L,k,s,p,d", [(4, 6, 33, 5, 1, 2, 1), (3, 8, 40, 3, 2, 1, 2), (17, 5, 12, 2, 1, 0, 1)])
def test_conv1d_rules(cin, cout, L, k, s, p, d):
    """Conv1d runs on the Conv2d kernels (one row): input rule and weight rule through the backend dispatch."""
    from vivit_amd.backend.extensions import _jac_t_mat_prod, _param_factor

    g = torch.Generator(device=DEV).manual_seed(6)
    N, Vd = 4, 3
    conv = nn.Conv1d(cin, cout, k, stride=s, padding=p, dilation=d).to(DEV)
    x = torch.randn(N, cin, L, generator=g, device=DEV)
    y = conv(x)
    M = torch.randn(Vd, *y.shape, generator=g, device=DEV)
    close(_jac_t_mat_prod(conv, M, x), jac_t_by_autograd(conv, x, M), rtol=1e-4, atol=1e-5)
    gotw = _param_factor(conv, "weight", M, x)
    ref = torch.empty_like(gotw)
    for v in range(Vd):
        for n in range(N):
            ref[v, n] = torch.autograd.grad(F.conv1d(x[n:n + 1], conv.weight, None, conv.stride, conv.padding, conv.dilation),
                                            conv.weight, grad_outputs=M[v, n:n + 1])[0]
    close(gotw, ref, rtol=1e-4, atol=1e-5 * math.sqrt(y.shape[2]))
    close(_param_factor(conv, "bias", M, x), M.sum(3), rtol=1e-5, atol=1e-5 * math.sqrt(y.shape[2]))


def test_linear_extra_dims_input_rule():
    from vivit_amd.backend.extensions import _jac_t_mat_prod

    g = torch.Generator(device=DEV).manual_seed(7)
    lin = nn.Linear(13, 9).to(DEV)
    x = torch.randn(5, 3, 4, 13, generator=g, device=DEV)
    M = torch.randn(2, 5, 3, 4, 9, generator=g, device=DEV)
    close(_jac_t_mat_prod(lin, M, x), jac_t_by_autograd(lin, x, M), rtol=1e-4, atol=1e-5)


def test_batchnorm_rules():
    from vivit_amd import kernels
    from vivit_amd.backend.extensions import _jac_t_mat_prod, _param_factor

    g = torch.Generator(device=DEV).manual_seed(3)
    bn = nn.BatchNorm2d(7).to(DEV).eval()
    bn.running_mean.uniform_(-0.5, 0.5)
    bn.running_var.uniform_(0.5, 1.5)
    bn.weight.data.uniform_(0.5, 1.5)
    bn.bias.data.uniform_(-0.5, 0.5)
    x = torch.randn(6, 7, 5, 4, generator=g, device=DEV)
    M = torch.randn(3, *x.shape, generator=g, device=DEV)
    close(_jac_t_mat_prod(bn, M, x), jac_t_by_autograd(bn, x, M))
    xhat = (x - bn.running_mean.view(1, -1, 1, 1)) / torch.sqrt(bn.running_var.view(1, -1, 1, 1) + bn.eps)
    close(_param_factor(bn, "weight", M, x), (M * xhat).flatten(3).sum(3), rtol=1e-4, atol=1e-5)
    close(_param_factor(bn, "bias", M, x), M.flatten(3).sum(3), rtol=1e-4, atol=1e-5)
    scale = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
    close(kernels.channel_scale(M, scale), M * scale.view(1, 1, -1, 1, 1))


@pytest.mark.parametrize("N,C", [(8, 10), (33, 100), (5, 1000)])
def test_cross_entropy_factors(N, C):
    from vivit_amd import kernels

    g = torch.Generator(device=DEV).manual_seed(4)
    logits = torch.randn(N, C, generator=g, device=DEV) * 3
    S = kernels.ce_sqrt_hessian(logits, 1.0 / math.sqrt(N))
    ref = oracle.loss_hessian_sqrt_exact(logits.cpu().double(), "ce")
    close(S.cpu().double(), ref, rtol=1e-4, atol=1e-6)
    # S S^T (over the slices) is the Hessian of the mean loss: diag(p) - p p^T, per sample
    p = logits.double().softmax(1)
    H = torch.einsum("vnc,vnd->ncd", S.double(), S.double())
    close(H, (torch.diag_embed(p) - p.unsqueeze(2) * p.unsqueeze(1)) / N, rtol=1e-4, atol=1e-6)
    # sampled factor with supplied one-hots
    idx = torch.multinomial(logits.softmax(1), 3, replacement=True, generator=g)
    onehot = F.one_hot(idx.t(), C).float()
    Smc = kernels.ce_sqrt_hessian(logits, 1.0 / math.sqrt(3 * N), onehot=onehot)
    close(Smc.cpu().double(), oracle.loss_hessian_sqrt_mc(logits.cpu().double(), onehot.cpu().double()), rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("n", [1, 5, 256, 257, 1000])
def test_pack_unpack_lower(n):
    from vivit_amd import kernels

    g = torch.Generator(device=DEV).manual_seed(5)
    A = torch.randn(n, n, generator=g, device=DEV)
    Gm = A + A.T
    packed = kernels.pack_lower(Gm)
    i, j = torch.tril_indices(n, n, device=DEV)
    assert torch.equal(packed, Gm[i, j])
    out = torch.full((n, n), float("nan"), device=DEV)
    kernels.unpack_lower_(packed, out)
    assert torch.equal(out, Gm)
    # a padded leading dimension on the source
    big = torch.zeros(n, n + 3, device=DEV)
    big[:, :n] = Gm
    assert torch.equal(kernels.pack_lower(big[:, :n]), packed)


# ---- edges of the factor rules (tests/epilogue_refs.py holds the grids; tests/test_epilogue_refs_host.py states what torch's
# fp64 CPU autograd gives on them) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["relu", "sigmoid", "tanh", "leaky_relu", "logsigmoid", "elu", "selu"])
def test_activation_rules_edge_grid(kind):
    """x on the grid {0, -0, +-1e-30 .. +-1e4, +-inf, NaN} against fp64 CPU autograd of the torch module: every entry in the
    same class (finite, inf or NaN), an exactly zero reference exactly zero here, finite entries at the tolerance of
    test_activation_rules.  (A zero class of its own cannot be asked of fp32: sigmoid'(20) = 2e-9 in fp64 is 0 in fp32
    because 1 + e^-20 rounds to 1; the implication tested is reference == 0  =>  result == 0.)"""
    from vivit_amd import kernels

    g = torch.Generator().manual_seed(8)
    x = R.act_grid_input()
    M = torch.randn(3, *x.shape, generator=g) + 2.0 * torch.sign(torch.randn(3, *x.shape, generator=g))   # |M| away from 0
    ref = R.act_reference(kind, x, M)
    got = kernels.act_jac_t(M.to(DEV), x.to(DEV), kind, R.ACT_PARAM.get(kind, 0.0)).cpu().double()
    assert torch.equal(got.isnan(), ref.isnan()), "NaN entries differ"
    assert torch.equal(got.isinf(), ref.isinf()), "inf entries differ"
    assert bool((got[ref == 0] == 0).all()), "a zero of the reference is not zero"
    fin = ref.isfinite()
    close(got[fin], ref[fin], rtol=2e-5, atol=1e-6)


def test_activation_rule_grid_stride():
    """More than 262 144 x 256 = 67 108 864 elements: the second trip of the grid-stride loop.  ReLU: bit-exact."""
    from vivit_amd import kernels

    V, per_v = 3, 22_400_000
    assert V * per_v > 262144 * 256
    g = torch.Generator(device=DEV).manual_seed(9)
    x = torch.randn(per_v // 100, 100, generator=g, device=DEV)
    M = torch.randn(V, *x.shape, generator=g, device=DEV)
    got = kernels.act_jac_t(M, x, "relu")
    ok = torch.equal(got, M * (x > 0))
    del got, M
    torch.cuda.empty_cache()
    assert ok


@pytest.mark.parametrize("V,N,C,sp", [(2, 3, 5, ()), (2, 3, 1, (4, 3)), (1, 1, 7, (13,)), (3, 2, 1, ())],
                         ids=["L=1", "C=1", "prime-CL", "C=1-L=1"])
def test_channel_scale_edges(V, N, C, sp):
    from vivit_amd import kernels

    g = torch.Generator(device=DEV).manual_seed(10)
    M = torch.randn(V, N, C, *sp, generator=g, device=DEV)
    scale = torch.randn(C, generator=g, device=DEV)
    got = kernels.channel_scale(M, scale)
    assert torch.equal(got, M * scale.view(1, 1, C, *([1] * len(sp))))


@pytest.mark.parametrize("plane", ["constant", "neg-inf", "one-nan"])
@pytest.mark.parametrize("shape,k,s,p", [((3, 2, 8, 8), 2, 2, 0), ((2, 3, 7, 9), 3, 2, 1)] + R.POOL_EDGE_GEOMS[:2])
def test_pooling_rules_special_planes(shape, k, s, p, plane):
    """A constant plane (every window tied: the first position in scan order takes the gradient), a plane of -inf and a plane
    with one NaN (the NaN is its windows' maximum), against torch autograd on the same device; input positions outside every
    window get exactly 0."""
    from vivit_amd import kernels

    g = torch.Generator(device=DEV).manual_seed(12)
    x = torch.randn(*shape, generator=g, device=DEV)
    if plane == "constant":
        x[0, 0] = 0.75
        x[1, 1] = 0.0
    elif plane == "neg-inf":
        x[0, 0] = float("-inf")
        x[1, 1, 2:5, 1:4] = float("-inf")
    else:
        x[0, 0, 3, 3] = float("nan")
        x[1, 1, 0, 0] = float("nan")
    unc = R.pool_uncovered(shape[2], shape[3], k, s, p).to(DEV)
    mod = nn.MaxPool2d(k, s, p)
    y = mod(x)
    M = torch.randn(2, *y.shape, generator=g, device=DEV)
    ref = jac_t_by_autograd(mod, x, M)
    got = kernels.maxpool2d_jac_t(M, x, R.pair(k), R.pair(s), R.pair(p))
    close(got, ref)
    assert bool((got[..., unc] == 0).all())
    mod = nn.AvgPool2d(k, s, p)
    got = kernels.avgpool2d_jac_t(M, x.shape[2:], R.pair(k), R.pair(s), R.pair(p))
    close(got, jac_t_by_autograd(mod, x, M))
    assert bool((got[..., unc] == 0).all())


@pytest.mark.parametrize("shape,k,s,p", R.POOL_EDGE_GEOMS)
def test_pooling_rules_uncovered_positions(shape, k, s, p):
    from vivit_amd import kernels

    g = torch.Generator(device=DEV).manual_seed(13)
    x = torch.randn(*shape, generator=g, device=DEV)
    unc = R.pool_uncovered(shape[2], shape[3], k, s, p).to(DEV)
    y = nn.MaxPool2d(k, s, p)(x)
    M = torch.randn(2, *y.shape, generator=g, device=DEV).abs() + 0.5
    assert bool((kernels.maxpool2d_jac_t(M, x, R.pair(k), R.pair(s), R.pair(p))[..., unc] == 0).all())
    avg = kernels.avgpool2d_jac_t(M, x.shape[2:], R.pair(k), R.pair(s), R.pair(p))
    assert bool((avg[..., unc] == 0).all()) and bool((avg[..., ~unc] != 0).all())


def _ce_checks(logits, N, C):
    from vivit_amd import kernels

    S = kernels.ce_sqrt_hessian(logits, 1.0 / math.sqrt(N))
    ref = oracle.loss_hessian_sqrt_exact(logits.cpu().double(), "ce")
    close(S.cpu().double(), ref, rtol=1e-4, atol=1e-6)
    del ref
    p = logits.double().softmax(1)
    H = torch.einsum("vnc,vnd->ncd", S.double(), S.double())
    close(H, (torch.diag_embed(p) - p.unsqueeze(2) * p.unsqueeze(1)) / N, rtol=1e-4, atol=1e-6)
    del H
    return S


@pytest.mark.parametrize("C", [1, 2, 255, 256, 257, 15360])
def test_cross_entropy_factor_class_counts(C):
    """C around the workgroup size (256) and at the LDS limit C * 4 = 60 KiB."""
    from vivit_amd import kernels

    N = 1 if C > 1000 else 5
    g = torch.Generator(device=DEV).manual_seed(14)
    logits = torch.randn(N, C, generator=g, device=DEV) * 3
    S = _ce_checks(logits, N, C)
    del S
    torch.cuda.empty_cache()
    idx = torch.multinomial(logits.softmax(1), 3, replacement=True, generator=g)
    onehot = F.one_hot(idx.t(), C).float()
    Smc = kernels.ce_sqrt_hessian(logits, 1.0 / math.sqrt(3 * N), onehot=onehot)
    close(Smc.cpu().double(), oracle.loss_hessian_sqrt_mc(logits.cpu().double(), onehot.cpu().double()), rtol=1e-4, atol=1e-6)


def test_cross_entropy_factor_refuses_too_many_classes():
    from vivit_amd import _lib, kernels

    logits = torch.zeros(1, 15361, device=DEV)
    onehot = torch.zeros(1, 1, 15361, device=DEV)
    with pytest.raises(_lib.VivitHipError) as exc:
        kernels.ce_sqrt_hessian(logits, 1.0, onehot=onehot)
    assert exc.value.status == _lib.VIVIT_E_UNSUPPORTED


@pytest.mark.parametrize("case", ["one-dominant", "all-equal", "masked", "all-very-negative"])
@pytest.mark.parametrize("C", [10, 257])
def test_cross_entropy_factor_logit_edges(C, case):
    from vivit_amd import kernels

    N = 6
    g = torch.Generator(device=DEV).manual_seed(15)
    logits = torch.randn(N, C, generator=g, device=DEV)
    if case == "one-dominant":
        logits[torch.arange(N), torch.arange(N) % C] = 1e4
    elif case == "all-equal":
        logits[:] = 2.5
    elif case == "masked":
        logits[:, 3] = float("-inf")
    else:
        logits -= 1e4
    S = _ce_checks(logits, N, C)
    assert bool(S.isfinite().all())
    if case == "masked":   # a masked class: its slice and its column are exactly 0
        assert bool((S[3] == 0).all()) and bool((S[:, :, 3] == 0).all())
    idx = torch.multinomial(logits.softmax(1), 3, replacement=True, generator=g)
    onehot = F.one_hot(idx.t(), C).float()
    Smc = kernels.ce_sqrt_hessian(logits, 1.0 / math.sqrt(3 * N), onehot=onehot)
    close(Smc.cpu().double(), oracle.loss_hessian_sqrt_mc(logits.cpu().double(), onehot.cpu().double()), rtol=1e-4, atol=1e-6)
