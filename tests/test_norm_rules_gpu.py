"""The LayerNorm / GroupNorm kernels (vivit_norm_stats_f32, vivit_norm_rules_f32, vivit_norm_position_sums_f32) and the GELU / SiLU
kinds of vivit_act_jac_t_f32 at their edge shapes, against fp64 references under the derived bounds of tests/norm_refs.py.

Row lengths: 1 (zero variance), 3, 64 | 65 (one element per lane and one more), 255 | 256 (scalar | 16-byte body), 1027 and 4100
(the workgroup route, ragged and multi-trip); segment lengths 1, 3 and 49 (segments that straddle lanes and waves) at row lengths
that are multiples of them on both routes and in both bodies; G in {1, 2, C}."""
import pytest
import torch

import norm_refs as R
from vivit_amd import _lib, kernels

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LN_EPS = 1e-5
ROW_L = [1, 3, 64, 65, 255, 256, 1027, 4100]
# (L, S, G): S = 1 is LayerNorm; L = S is G = C (one channel per group)
RULE_CASES = [(L, 1, 1) for L in ROW_L] + [(3, 3, 2), (49, 49, 3), (255, 3, 2), (98, 49, 1), (196, 49, 2), (1029, 3, 1), (1032, 3, 2),
                                           (1176, 49, 2), (4100, 4, 1)]


def check(got, ref, bound, what):
    ok, msg = R.within(got.cpu(), ref, bound)
    assert ok, f"{what}: {msg}"


def fp32_stats(x, eps=LN_EPS):
    """fp32 mean / rstd for the rules tests: the fp64 statistics rounded (the rules take them as inputs)."""
    mean, rstd = R.stats(x, eps)
    return mean.float(), rstd.float()


def run_rules(M, x, gamma, mean, rstd, G, S, want=(True, True, True), shift=False):
    dev = lambda t: None if t is None else (R.misaligned(t.to(DEV)) if shift else t.to(DEV))   # noqa: E731
    return kernels.norm_rules(dev(M), x.to(DEV), gamma.to(DEV) if gamma is not None else None, mean.to(DEV), rstd.to(DEV), G, S, want)


@pytest.mark.parametrize("shift", [False, True], ids=["aligned", "offset4"])
@pytest.mark.parametrize("L", ROW_L)
def test_norm_stats(L, shift):
    rows = 5
    x = R.generic(R.gen(L), rows, L)
    xd = R.misaligned(x.to(DEV)) if shift else x.to(DEV)
    mean, rstd = kernels.norm_stats(xd, rows, LN_EPS)
    rm, rr = R.stats(x, LN_EPS)
    bm, br = R.stats_bounds(x, LN_EPS, vec=L % 4 == 0 and not shift)
    check(mean, rm, bm, "mean")
    check(rstd, rr, br, "rstd")
    m2, r2 = kernels.norm_stats(xd, rows, LN_EPS)
    assert torch.equal(mean, m2) and torch.equal(rstd, r2)


@pytest.mark.parametrize("L", [3, 64, 255, 256, 1027, 4100])
def test_norm_stats_offset_data(L):
    """x = 1000 + 0.1 noise: the two-pass variance keeps rstd within 1e-3 of fp64 (the error of the fp32 mean, about
    log L * 2^-24 * 1000, enters to second order); E[x^2] - mean^2 in fp32 would miss this by orders of magnitude."""
    g = R.gen(7 + L)
    x = (1000.0 + 0.1 * torch.randn(6, L, generator=g, dtype=R.F64)).float()
    mean, rstd = kernels.norm_stats(x.to(DEV), 6, LN_EPS)
    rm, rr = R.stats(x, LN_EPS)
    rel = ((rstd.cpu().double() - rr) / rr).abs().max().item()
    print(f"L={L}: rstd relative error {rel:.3g}, mean error {(mean.cpu().double() - rm).abs().max().item():.3g}")
    assert rel <= 1e-3


@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("L,S,G", RULE_CASES)
def test_norm_rules(L, S, G, V):
    rows = 2 * G
    M, x, gamma = R.make_rows(L * 31 + S + G + V, V, rows, L, G, S)
    mean, rstd = fp32_stats(x)
    refs, mags = R.rules(M, x, gamma, mean, rstd, G, S)
    bounds = R.rules_bounds(mags, L, S, vec=L % 4 == 0)
    got = run_rules(M, x, gamma, mean, rstd, G, S)
    for name, g_, r_, b_ in zip(("out", "seg_w", "seg_b"), got, refs, bounds):
        check(g_.view(r_.shape), r_, b_, f"{name} L={L} S={S} G={G}")
    if L == 1:   # var = 0: xhat = 0 and h - mean(h) = 0 exactly
        assert torch.count_nonzero(got[0]) == 0
    if S == 1:
        assert torch.equal(got[2].view(M.shape).cpu(), M)
    # gamma = None is gamma = 1
    refs1, mags1 = R.rules(M, x, None, mean, rstd, G, S)
    out1 = run_rules(M, x, None, mean, rstd, G, S, want=(True, False, False))[0]
    check(out1.view(refs1[0].shape), refs1[0], R.rules_bounds(mags1, L, S, vec=L % 4 == 0)[0], "out without gamma")


@pytest.mark.parametrize("L,S,G", [(256, 1, 1), (4100, 1, 1), (196, 49, 2), (1032, 3, 2)])
def test_norm_rules_offset_pointer(L, S, G):
    """M four bytes off a 16-byte boundary: the scalar body."""
    rows = 2 * G
    M, x, gamma = R.make_rows(L + S, 2, rows, L, G, S)
    mean, rstd = fp32_stats(x)
    refs, mags = R.rules(M, x, gamma, mean, rstd, G, S)
    got = run_rules(M, x, gamma, mean, rstd, G, S, shift=True)
    for name, g_, r_, b_ in zip(("out", "seg_w", "seg_b"), got, refs, R.rules_bounds(mags, L, S, vec=False)):
        check(g_.view(r_.shape), r_, b_, name)


def test_norm_rules_offset_input_with_statistics_of_the_kernel():
    """x = 1000 + 0.1 noise through both launches: statistics from vivit_norm_stats_f32, rules on them."""
    L, rows = 1027, 3
    g = R.gen(3)
    M = R.generic(g, 2, rows, L)
    x = (1000.0 + 0.1 * torch.randn(rows, L, generator=g, dtype=R.F64)).float()
    mean, rstd = kernels.norm_stats(x.to(DEV), rows, LN_EPS)
    refs, mags = R.rules(M, x, None, mean.cpu(), rstd.cpu(), 1, 1)
    got = kernels.norm_rules(M.to(DEV), x.to(DEV), None, mean, rstd)
    check(got[0], refs[0], R.rules_bounds(mags, L, 1, vec=False)[0], "out")


@pytest.mark.parametrize("S,G", [(1, 1), (3, 2)])
def test_norm_rules_many_rows(S, G):
    """70 000 rows of three elements: beyond 65 535 in every grid dimension a launch could have used for them."""
    rows, L = 70000, 3
    M, x, gamma = R.make_rows(11 + S, 1, rows, L, G, S)
    mean, rstd = fp32_stats(x)
    refs, mags = R.rules(M, x, gamma, mean, rstd, G, S)
    got = run_rules(M, x, gamma, mean, rstd, G, S)
    for name, g_, r_, b_ in zip(("out", "seg_w", "seg_b"), got, refs, R.rules_bounds(mags, L, S, vec=False)):
        check(g_.view(r_.shape), r_, b_, name)
    km, kr = kernels.norm_stats(x.to(DEV), rows, LN_EPS)
    bm, br = R.stats_bounds(x, LN_EPS, vec=False)
    rm, rr = R.stats(x, LN_EPS)
    check(km, rm, bm, "mean")
    check(kr, rr, br, "rstd")


@pytest.mark.parametrize("skip", [0, 1, 2])
@pytest.mark.parametrize("L,S,G", [(65, 1, 1), (196, 49, 2), (1176, 49, 2), (4100, 1, 1)])
def test_norm_rules_null_outputs(L, S, G, skip):
    """One of out / seg_w / seg_b NULL: the other two bit for bit those of the full call."""
    rows = 2 * G
    M, x, gamma = R.make_rows(L, 2, rows, L, G, S)
    mean, rstd = fp32_stats(x)
    full = run_rules(M, x, gamma, mean, rstd, G, S)
    want = tuple(i != skip for i in range(3))
    part = run_rules(M, x, gamma, mean, rstd, G, S, want=want)
    for i in range(3):
        assert (part[i] is None) if i == skip else torch.equal(part[i], full[i])


@pytest.mark.parametrize("L,S,G", [(64, 1, 1), (255, 1, 1), (256, 1, 1), (1027, 1, 1), (4100, 1, 1), (196, 49, 2), (1176, 49, 2)])
def test_norm_rules_batch_independence(L, S, G):
    """The same row in two launches that differ in V, in the number of rows and in the row's position: equal bytes in all three
    results; and two runs of one launch are equal."""
    Ma, xa, gamma = R.make_rows(5 * L, 1, 2 * G, L, G, S)
    Mb, xb, _ = R.make_rows(5 * L + 1, 3, 5 * G, L, G, S)
    ra, (vb, rb) = G - 1, (2, 3 * G + G - 1)          # same row % G: the same gamma
    Mb[vb, rb], xb[rb] = Ma[0, ra], xa[ra]
    ma, sa = fp32_stats(xa)
    mb, sb = fp32_stats(xb)
    mb[rb], sb[rb] = ma[ra], sa[ra]
    A = run_rules(Ma, xa, gamma, ma, sa, G, S)
    B = run_rules(Mb, xb, gamma, mb, sb, G, S)
    B2 = run_rules(Mb, xb, gamma, mb, sb, G, S)
    for a, b, b2 in zip(A, B, B2):
        assert torch.equal(a.view(1, 2 * G, -1)[0, ra], b.view(3, 5 * G, -1)[vb, rb])
        assert torch.equal(b, b2)
    # the statistics of the row as well
    ka, kb = kernels.norm_stats(xa.to(DEV), 2 * G, LN_EPS), kernels.norm_stats(xb.to(DEV), 5 * G, LN_EPS)
    assert ka[0][ra] == kb[0][rb] and ka[1][ra] == kb[1][rb]


@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("A", [1, 5])
@pytest.mark.parametrize("D", [3, 256, 300])
def test_norm_position_sums(D, A, V):
    N = 3
    g = R.gen(D + 10 * A + V)
    M, x = R.generic(g, V, N, A, D), R.generic(g, N, A, D)
    mean, rstd = fp32_stats(x.view(N * A, D))
    (rw, rb), (bw, bb) = R.position_sums(M, x, mean, rstd)
    pw, pb = kernels.norm_position_sums(M.to(DEV), x.to(DEV), mean.to(DEV), rstd.to(DEV))
    check(pw, rw, bw, "pw")
    check(pb, rb, bb, "pb")
    # sample 1 alone (V = 1, N = 1): the same bytes
    pw1, pb1 = kernels.norm_position_sums(M[V - 1:, 1:2].to(DEV), x[1:2].to(DEV), mean[A:2 * A].to(DEV), rstd[A:2 * A].to(DEV))
    assert torch.equal(pw1[0, 0], pw[V - 1, 1]) and torch.equal(pb1[0, 0], pb[V - 1, 1])


def test_norm_launchers_refuse_bad_arguments():
    M, x = torch.zeros(2, 4, 6, device=DEV), torch.zeros(4, 6, device=DEV)
    mean = rstd = torch.zeros(4, device=DEV)
    with pytest.raises(ValueError):
        kernels.norm_rules(M, x[:3], None, mean, rstd)
    with pytest.raises(ValueError):
        kernels.norm_rules(M, x, None, mean, rstd, seg=4)
    with pytest.raises(ValueError):
        kernels.norm_rules(M, x, torch.zeros(5, device=DEV), mean, rstd)
    with pytest.raises(ValueError):
        kernels.norm_position_sums(M, x, mean, rstd)
    with pytest.raises(RuntimeError):
        kernels.norm_stats(x.cpu(), 4, 1e-5)
    lib = _lib.load()
    assert lib.vivit_norm_rules_f32(M.data_ptr(), x.data_ptr(), None, mean.data_ptr(), rstd.data_ptr(), None, None, None, 2, 4, 6, 1, 1,
                                    None) == _lib.VIVIT_E_BADARG
    assert lib.vivit_norm_rules_f32(M.data_ptr(), x.data_ptr(), None, mean.data_ptr(), rstd.data_ptr(), M.data_ptr(), None, None, 2, 4, 6, 3,
                                    1, None) == _lib.VIVIT_E_BADARG   # rows % G


# ---- GELU and SiLU ----------------------------------------------------------------------------------------------------------------------
ACT_KINDS = ["gelu", "gelu_tanh", "silu"]


@pytest.mark.parametrize("kind", ACT_KINDS)
def test_activation_derivative_on_a_grid(kind):
    x = torch.cat([torch.linspace(-12, 12, 4801), torch.tensor([-100.0, -50.0, -20.0, 20.0, 50.0, 100.0, 1e-30, -1e-30, 0.0])])
    M = torch.ones(1, x.numel())
    got = kernels.act_jac_t(M.to(DEV), x.to(DEV), kind)[0]
    ref, bound = R.act_derivative(kind, x)
    check(got, ref, bound, kind)
    # and as a factor: M [V, N, F] against M f'(x), one more rounding
    g = R.gen(1)
    Mv, xv = R.generic(g, 3, 4, 50), torch.randn(4, 50, generator=g) * 3
    rv, bv = R.act_derivative(kind, xv)
    got = kernels.act_jac_t(Mv.to(DEV), xv.to(DEV), kind)
    check(got, Mv.double() * rv, Mv.double().abs() * (bv + R.EPS * rv.abs()), kind + " factor")


@pytest.mark.parametrize("kind", ACT_KINDS)
def test_activation_edges_as_torch(kind):
    """0, +-1e-30, +-10, +-100, +-inf, NaN against torch's CPU fp32 autograd of the module: the same finite / NaN class, and finite
    values within the sum of both sides' bounds."""
    inf, nan = float("inf"), float("nan")
    x = torch.tensor([0.0, 1e-30, -1e-30, 10.0, -10.0, 100.0, -100.0, inf, -inf, nan])
    xr = x.clone().requires_grad_(True)
    (ref,) = torch.autograd.grad(R.act_module(kind)(xr).sum(), xr)
    got = kernels.act_jac_t(torch.ones(1, x.numel(), device=DEV), x.to(DEV), kind)[0].cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(torch.isinf(got), torch.isinf(ref))
    fin = torch.isfinite(ref)
    _, bound = R.act_derivative(kind, x[fin])
    check(got[fin], ref[fin].double(), 2 * bound, kind)
