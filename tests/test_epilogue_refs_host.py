"""Host checks of tests/epilogue_refs.py (no GPU): the exactness precondition of every exact-family case the GPU tests
use, the agreement of tests/helpers.py::OracleBackend (which the host flavour of the API tests trusts) with the new fp64
references, and the values torch's fp64 CPU autograd gives at the activation and pooling edges of the GPU tests."""
import math

import pytest
import torch
from torch import nn

import epilogue_refs as R
from helpers import OracleBackend

F64 = torch.float64


def assert_exact_case(ref, mag):
    """``ref``: fp64 reference of an exact-family case; ``mag``: the same formula on absolute values (sum of |terms|, which
    bounds every partial sum in any order).  The fp32 result is then order-independent and equals ``ref``."""
    assert float(mag.max()) < 2 ** 24
    assert bool((ref.abs() <= mag).all())
    scaled = ref * 2.0 ** 12
    assert torch.equal(scaled, scaled.round()), "not dyadic with 12 fractional bits"
    assert torch.equal(ref.float().double(), ref), "round trip through fp32 loses bits"


def absall(*ts):
    return [t.abs() for t in ts]


# ---- exactness precondition ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,N", R.HADAMARD_SHAPES)
def test_exact_hadamard(C, N):
    Gz, Gs, G0 = R.make_hadamard("exact", C, N)
    for alpha, beta in R.HADAMARD_AB:
        assert_exact_case(R.hadamard(Gz, Gs, C, N, alpha, beta, G0), R.hadamard(*absall(Gz, Gs), C, N, abs(alpha), abs(beta), G0.abs()))


@pytest.mark.parametrize("name,Cr,Nr,Cc,Nc", R.HADAMARD_BLOCK_SHAPES)
def test_exact_hadamard_block(name, Cr, Nr, Cc, Nc):
    Gz, Gs, G0 = R.make_hadamard_block("exact", Cr, Nr, Cc, Nc)
    for alpha, beta in [(1.0, 0.0), (0.5, 1.0)]:
        assert_exact_case(R.hadamard_block(Gz, Gs, Cr, Nr, Cc, Nc, alpha, beta, G0),
                          R.hadamard_block(*absall(Gz, Gs), Cr, Nr, Cc, Nc, alpha, abs(beta), G0.abs()))


@pytest.mark.parametrize("F,C,N,O", R.CLASS_SHAPES)
def test_exact_class(F, C, N, O):
    mat, s, U = R.make_class("exact", F, C, N, O)
    assert_exact_case(R.class_contract(mat, s), R.class_contract(mat.abs(), s.abs()))
    assert_exact_case(R.class_expand(s, U), R.class_expand(s.abs(), U.abs()))


@pytest.mark.parametrize("C,N,K", R.DIR_CURV_SHAPES)
def test_exact_dir_curvature(C, N, K):
    GE, ev = R.make_dir_curvature("exact", C, N, K)
    ref = R.dir_curvature(GE, ev, C, N, 0.25)
    assert_exact_case(ref, ref)   # (all terms non-negative)
    assert float((GE.double() ** 2).reshape(C, N, K).sum(0).max()) < 2 ** 24   # the sum before the division


@pytest.mark.parametrize("rows,K,ldx", R.SCALE_COLS_SHAPES)
def test_exact_scale_cols(rows, K, ldx):
    X, ev = R.make_scale_cols("exact", rows, K)
    for pre in (1.0, 0.5):
        assert_exact_case(R.scale_cols_rsqrt(X, ev, pre), R.scale_cols_rsqrt(X.abs(), ev, pre))
    assert torch.equal(ev.double().sqrt() ** 2, ev.double())   # 4^j: the square root is a power of two


@pytest.mark.parametrize("K,lens", R.NORMALIZE_SHAPES)
def test_exact_row_sqnorm(K, lens):
    ts = R.make_normalize("exact", K, lens)
    acc0 = (torch.arange(K) % 1000).float()
    ref = R.row_sqnorm(ts, acc0)
    assert_exact_case(ref, ref)
    assert float(R.row_sqnorm(ts).min()) > 0


@pytest.mark.parametrize("L", list(R.ROW_L))
def test_exact_row_dot_and_bn(L):
    for rows in R.ROW_ROWS:
        M, X = R.make_rows("exact", rows, rows, L)
        assert_exact_case(R.row_dot(M, X, rows), R.row_dot(M.abs(), X.abs(), rows))
        assert_exact_case(R.row_dot(M), R.row_dot(M.abs()))
    M, X = R.make_rows("exact", 12, 4, L)
    assert_exact_case(R.row_dot(M, X, 4), R.row_dot(M.abs(), X.abs(), 4))
    for C in (1, 7):
        for V in (1, 3):
            M, x, scale, mean, rstd = R.make_bn("exact", V, 2, C, L)
            out, mx, ms = R.bn_eval_rules(M, x, scale)
            aout, amx, ams = R.bn_eval_rules(M.abs(), x.abs(), scale)
            for ref, mag in ((out, aout), (mx, amx), (ms, ams)):
                assert_exact_case(ref, mag)
            w = R.bn_eval_rules(M, x, scale, mean, rstd)[1]
            assert_exact_case(w, R.bn_eval_rules(M.abs(), x.abs(), scale, -mean.abs(), rstd)[1])


@pytest.mark.parametrize("name,C,N,O,I", R.LINEAR_MJP_SHAPES)
def test_exact_linear_mjp(name, C, N, O, I):
    s, z = R.make_linear_mjp("exact", C, N, O, I)
    assert_exact_case(R.linear_weight_mjp(s, z), R.linear_weight_mjp(s.abs(), z.abs()))


def test_exact_linear_mjp_stride_case():
    """The stride case has no sums: a single product of two integers of magnitude <= 4 per element (not materialised here)."""
    s, z = R.make_linear_mjp("exact", *R.LINEAR_MJP_STRIDE)
    for t in (s, z):
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= 4


@pytest.mark.parametrize("n", R.SYMM_N)
def test_symmetrize_case(n):
    buf, view = R.make_symm(n, n + 3)
    ref = R.symmetrize_lower(view)
    assert torch.equal(ref, ref.T) and not bool(ref.isnan().any())
    assert torch.equal(torch.tril(ref), torch.tril(view.double()))
    assert R.padding_untouched(buf, n)


def test_builders():
    t = torch.arange(24.0).reshape(2, 3, 4)
    m = R.misaligned(t)
    assert torch.equal(m, t) and m.data_ptr() % 16 == 4 and m.is_contiguous()
    buf, view = R.with_sentinel_padding(3, 4, 7)
    assert view.shape == (3, 4) and view.data_ptr() == buf.data_ptr() and R.padding_untouched(buf, 4)
    view.fill_(1.0)
    assert R.padding_untouched(buf, 4)
    buf[1, 5] = 0.0
    assert not R.padding_untouched(buf, 4)
    g = R.generic(R.gen(0), 10000).abs()
    assert float(g.max() / g.median()) > 30   # magnitudes spread over orders


# ---- the oracle backend of the host API tests against the new references ---------------------------------------------------
def close64(a, b):
    torch.testing.assert_close(a.to(F64), b, rtol=1e-13, atol=0.0)


def test_oracle_backend_agrees():
    ob = OracleBackend()
    d = lambda *ts: [t.double() for t in ts]   # noqa: E731
    C, N = 3, 7
    Gz, Gs, G0 = d(*R.make_hadamard("generic", C, N))
    close64(ob.gram_hadamard(Gz, Gs, C, N), R.hadamard(Gz, Gs, C, N))
    close64(ob.gram_hadamard(Gz, Gs, C, N, out=G0.clone(), alpha=0.25, beta=-0.5), R.hadamard(Gz, Gs, C, N, 0.25, -0.5, G0))
    for _, Cr, Nr, Cc, Nc in R.HADAMARD_BLOCK_SHAPES[:4]:
        Gz, Gs, G0 = d(*R.make_hadamard_block("generic", Cr, Nr, Cc, Nc))
        close64(ob.gram_hadamard_block(Gz, Gs, Cr, Nr, Cc, Nc), R.hadamard_block(Gz, Gs, Cr, Nr, Cc, Nc))
        close64(ob.gram_hadamard_block(Gz, Gs, Cr, Nr, Cc, Nc, out=G0.clone(), alpha=2.0, beta=1.0),
                R.hadamard_block(Gz, Gs, Cr, Nr, Cc, Nc, 2.0, 1.0, G0))
    for F, Cc, Nn, O in R.CLASS_SHAPES[:4]:
        mat, s, U = d(*R.make_class("generic", F, Cc, Nn, O))
        close64(ob.class_contract(mat, s), R.class_contract(mat, s))
        close64(ob.class_expand(s, U), R.class_expand(s, U))
    for Cc, Nn, K in R.DIR_CURV_SHAPES[:3]:
        GE, ev = d(*R.make_dir_curvature("generic", Cc, Nn, K))
        close64(ob.dir_curvature(GE, ev, Cc, Nn, 0.3), R.dir_curvature(GE, ev, Cc, Nn, 0.3))
    X, ev = d(*R.make_scale_cols("generic", 6, 4))
    got = ob.scale_cols_rsqrt_(X.clone(), ev, pre=0.7)
    close64(got, R.scale_cols_rsqrt(X, ev, 0.7))
    ts = d(*R.make_normalize("generic", 16, (3, 20000)))
    ts = [ts[0], ts[1].reshape(16, 200, 100)]
    got = ob.normalize_rows_([t.clone() for t in ts])
    for a, b in zip(got, R.normalize_rows(ts)):
        close64(a, b)
    s, z = d(*R.make_linear_mjp("generic", 3, 5, 4, 7))
    close64(ob.linear_weight_mjp(s, z), R.linear_weight_mjp(s, z))


# ---- activation edges: what torch's fp64 CPU autograd gives on the grid of the GPU test -----------------------------------
def test_activation_edge_values():
    inf, nan = R.INF, R.NAN
    sa = R.SELU_SCALE * R.SELU_ALPHA
    # the derivative at +0 and -0 of the piecewise rules: the branch of x <= 0
    for kind, at0 in (("relu", 0.0), ("leaky_relu", 0.1), ("elu", 0.7), ("selu", sa)):
        got = R.act_derivative_fp64(kind, [0.0, -0.0])
        torch.testing.assert_close(got, torch.tensor([at0, at0], dtype=F64), rtol=1e-15, atol=0.0)
    # smooth rules at 0
    for kind, at0 in (("sigmoid", 0.25), ("tanh", 1.0), ("logsigmoid", 0.5)):
        assert R.act_derivative_fp64(kind, [0.0, -0.0]).tolist() == [at0, at0]
    # zeros beyond saturation (exactly 0 in fp64 as well)
    assert R.act_derivative_fp64("sigmoid", [1e4, -1e4, inf, -inf, 88.0, 104.0]).tolist() == [0.0] * 6
    assert R.act_derivative_fp64("tanh", [20.0, -20.0, 88.0, -88.0, 104.0, -104.0, 1e4, -1e4, inf, -inf]).tolist() == [0.0] * 10
    assert R.act_derivative_fp64("logsigmoid", [1e4, inf, -1e4, -inf]).tolist() == [0.0, 0.0, 1.0, 1.0]
    assert R.act_derivative_fp64("relu", [-1e-30, -inf, 1e-30, inf]).tolist() == [0.0, 0.0, 1.0, 1.0]
    assert R.act_derivative_fp64("elu", [-1e4, -inf, inf]).tolist() == [0.0, 0.0, 1.0]
    assert R.act_derivative_fp64("selu", [-1e4, -inf, inf]).tolist() == [0.0, 0.0, R.SELU_SCALE]
    torch.testing.assert_close(R.act_derivative_fp64("leaky_relu", [-1e4, -inf, inf]), torch.tensor([0.1, 0.1, 1.0], dtype=F64))
    # below saturation the fp64 derivative is tiny but not zero
    assert 0.0 < float(R.act_derivative_fp64("sigmoid", [-104.0])[0]) < 1e-44
    # NaN in: NaN out, except for ReLU and LeakyReLU.  Their backward kernels are selects on `x <= 0` and `x > 0`, which a
    # NaN fails: ReLU passes the gradient unchanged, LeakyReLU scales it by the negative slope.  (ELU and SELU: NaN from
    # the vectorised loop of torch's CPU kernel -- what act_reference pins -- but the positive-side factor from its scalar
    # remainder loop, which a short tensor runs.)
    for kind in ("sigmoid", "tanh", "logsigmoid", "elu", "selu"):
        assert math.isnan(float(R.act_derivative_fp64(kind, [nan])[0]))
    for kind, at_nan in (("relu", 1.0), ("leaky_relu", 0.1)):
        torch.testing.assert_close(R.act_derivative_fp64(kind, [nan]), torch.tensor([at_nan], dtype=F64), rtol=1e-15, atol=0.0)
    x = R.act_grid_input()
    assert x.shape == (4, 3 * len(R.ACT_GRID)) and int(x.isnan().sum()) == 12


# ---- pooling edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,k,s,p", R.POOL_EDGE_GEOMS)
def test_pooling_uncovered_positions_get_zero(shape, k, s, p):
    g = R.gen(11)
    x = torch.randn(*shape, generator=g, dtype=F64)
    unc = R.pool_uncovered(shape[2], shape[3], k, s, p)
    if R.pair(s)[0] > R.pair(k)[0] or R.pair(s)[1] > R.pair(k)[1]:
        assert bool(unc.any())
    for mod in (nn.MaxPool2d(k, s, p), nn.AvgPool2d(k, s, p)):
        y = mod(x)
        M = torch.randn(2, *y.shape, generator=g, dtype=F64).abs() + 0.5
        grad = R.jac_t_by_autograd(mod, x, M)
        assert bool((grad[..., unc] == 0).all())
        if isinstance(mod, nn.AvgPool2d):
            assert bool((grad[..., ~unc] != 0).all())   # every covered position receives something


def test_pooling_special_planes():
    """MaxPool2d(2, 2) on a constant plane and on a plane of -inf sends each window's gradient to its first position; a NaN
    is the maximum of its window and takes that window's gradient."""
    mod = nn.MaxPool2d(2, 2)
    first = torch.zeros(4, 4, dtype=F64)
    first[::2, ::2] = 1.0
    for fill in (1.5, -R.INF):
        x = torch.full((1, 1, 4, 4), fill, dtype=F64)
        assert torch.equal(R.jac_t_by_autograd(mod, x, torch.ones(1, 1, 1, 2, 2, dtype=F64))[0, 0, 0], first)
    x = torch.arange(16.0, dtype=F64).reshape(1, 1, 4, 4)
    x[0, 0, 1, 0] = R.NAN
    want = torch.zeros(4, 4, dtype=F64)
    want[1, 0] = want[1, 3] = want[3, 1] = want[3, 3] = 1.0
    assert torch.equal(R.jac_t_by_autograd(mod, x, torch.ones(1, 1, 1, 2, 2, dtype=F64))[0, 0, 0], want)
