"""fp64 references and derived error bounds for the LayerNorm / GroupNorm kernels (csrc/norm_rules.hip) and the GELU / SiLU kinds of
``vivit_act_jac_t_f32``.  TEST INFRASTRUCTURE shared by tests/test_norm_rules_gpu.py; in the manner of tests/epilogue_refs.py.

Every reference restates the formula of include/vivit_hip.h in torch fp64.  The rules take ``mean`` and ``rstd`` as fp32 INPUTS, so
their references use the very fp32 values the kernel was given; the statistics have a test of their own.

Error bounds (eps = 2^-24, elementwise against the fp64 reference, first order in eps; derived, not fitted):

* A sum of fp32 terms t_i along any fixed tree has the running-error bound  depth * eps * sum |t_i|, depth = the number of additions
  on the longest path from a term to the result.  The kernels sum a row of L elements as: a serial sum per lane (T lanes; T = 64 on
  the wave route, L <= 1024, else 256), a butterfly over the 64 lanes of a wave (6 levels) and, on the workgroup route, the four wave
  sums one after the other (3).  :func:`sum_depth` counts exactly that: ceil(L / T) + log2(T) + O(1), i.e. the tree part grows with
  log T and the per-lane part is at most 16 terms on the wave route and L / 256 on the workgroup route (17 at L = 4100).
* xhat = (x - mean) * rstd: two roundings, |d xhat| <= 2 eps |xhat|.  h = gamma M: one rounding.
* c1 = sum(h) / L: (depth + 2) eps mean|h|  (one rounding per term for h, the division).
  c2 = sum(h xhat) / L: (depth + 5) eps mean|h xhat|  (h: 1, xhat: 2, the fused multiply-add: 1 with its addition counted in depth, the division: 1).
* out = rstd ((h - c1) - xhat c2): the errors of c1, c2, h and xhat propagate, plus one rounding each for the product xhat c2, the two
  subtractions and the final product.  Collecting the coefficient of every magnitude gives at most
      (depth + 10) eps |rstd| (|h| + mean|h| + |xhat| mean|h xhat|).
* seg_w = sum_s M xhat over a segment of S elements: W = min(64, 2^ceil(log2 S)) lanes, ceil(S / W) serial terms per lane, log2 W
  butterfly levels; every term carries 3 eps (xhat: 2, the multiply-add: 1): (ceil(S / W) + log2 W + 3) eps sum|M xhat|.  S = 1: a
  single product, 3 eps |M xhat|.  seg_b likewise without the 3 (S = 1: exact).
* position sums over A: serial, (A + 3) eps sum_a |M xhat| and A eps sum_a |M|.
* mean = sum(x) / L: E_mean = (depth + 1) eps mean|x|.  The two-pass variance sum (x - m)^2 / L with m = mean + d equals var + d^2
  EXACTLY in real arithmetic (sum (x - mean) = 0), so the mean's error enters to second order; its own rounding is (depth + 4) eps
  relative (subtraction 1, square 2 with the multiply-add, division 1).  rstd = 1 / sqrt(var + e) halves a relative error of its
  argument and adds 3 roundings (the addition, sqrt, the division):
      |d rstd| / rstd <= 0.5 (E_mean^2 / (var + e) + (depth + 4) eps) + 3 eps.
"""
import math

import torch

from epilogue_refs import EPS, F64, gen, generic, misaligned, within   # noqa: F401  (re-exported for the test module)

WAVE_L = 1024     # rows up to this length are held by one wavefront (NORM_WAVE_L of csrc/norm_rules.hip)
FLT_MIN = 2.0 ** -126


def sum_depth(L, vec):
    """Additions on the longest path of the kernels' sum over a row of ``L`` elements (``vec``: the 16-byte body)."""
    T = 64 if L <= WAVE_L else 256
    serial = 4 * math.ceil(L / (4 * T)) if vec else math.ceil(L / T)
    return serial + 6 + (3 if L > WAVE_L else 0)


def seg_depth(S):
    W = 1
    while W < S and W < 64:
        W *= 2
    return math.ceil(S / W) + int(math.log2(W))


# ---- statistics ---------------------------------------------------------------------------------------------------------------------
def stats(x, eps):
    """x [rows, L] -> (mean, rstd) in fp64, biased variance."""
    x = x.to(F64)
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    return mean, 1.0 / torch.sqrt(var + eps)


def stats_bounds(x, eps, vec):
    """(bound on |mean - ref|, bound on |rstd - ref|)."""
    x = x.to(F64)
    L = x.shape[1]
    d = sum_depth(L, vec)
    mean, rstd = stats(x, eps)
    var = ((x - mean[:, None]) ** 2).mean(1)
    e_mean = (d + 1) * EPS * x.abs().mean(1)
    rel = 0.5 * (e_mean ** 2 / (var + eps) + (d + 4) * EPS) + 3 * EPS
    return e_mean, rel * rstd


# ---- rules ----------------------------------------------------------------------------------------------------------------------------
def gamma_index(rows, L, G, S):
    """[rows, L] long: (row % G) (L / S) + l / S."""
    r = torch.arange(rows).view(rows, 1)
    l = torch.arange(L).view(1, L)
    return (r % G) * (L // S) + l // S


def rules(M, x, gamma, mean, rstd, G=1, S=1):
    """M [V, rows, L], x [rows, L], gamma [G L / S] or None, mean / rstd [rows] -> (out [V, rows, L], seg_w, seg_b [V, rows, L / S])
    and the same three evaluated on absolute values (the magnitudes the bounds are made of)."""
    V, rows, L = M.shape
    M, x, mean, rstd = M.to(F64), x.to(F64), mean.to(F64), rstd.to(F64)
    g = torch.ones(rows, L, dtype=F64) if gamma is None else gamma.to(F64)[gamma_index(rows, L, G, S)]
    xhat = (x - mean[:, None]) * rstd[:, None]
    h = g * M
    out = rstd[:, None] * (h - h.mean(2, keepdim=True) - xhat * (h * xhat).mean(2, keepdim=True))
    seg_w = (M * xhat).view(V, rows, L // S, S).sum(3)
    seg_b = M.view(V, rows, L // S, S).sum(3)
    mag_out = rstd.abs()[:, None] * (h.abs() + h.abs().mean(2, keepdim=True) + xhat.abs() * (h * xhat).abs().mean(2, keepdim=True))
    mag_w = (M * xhat).abs().view(V, rows, L // S, S).sum(3)
    mag_b = M.abs().view(V, rows, L // S, S).sum(3)
    return (out, seg_w, seg_b), (mag_out, mag_w, mag_b)


def rules_bounds(mags, L, S, vec):
    mag_out, mag_w, mag_b = mags
    ds = seg_depth(S) if S > 1 else 0
    return (sum_depth(L, vec) + 10) * EPS * mag_out, (ds + 3) * EPS * mag_w, ds * EPS * mag_b


def position_sums(M, x, mean, rstd):
    """M [V, N, A, D], x [N, A, D], mean / rstd [N A] -> (pw, pb) [V, N, D] and their bounds."""
    V, N, A, D = M.shape
    M, x = M.to(F64), x.to(F64)
    xhat = (x - mean.to(F64).view(N, A, 1)) * rstd.to(F64).view(N, A, 1)
    pw, pb = (M * xhat).sum(2), M.sum(2)
    return (pw, pb), ((A + 3) * EPS * (M * xhat).abs().sum(2), A * EPS * M.abs().sum(2))


def make_rows(seed, V, rows, L, G=1, S=1, affine=True, offset=0.0):
    """Seeded operands (CPU fp32): M [V, rows, L], x [rows, L], gamma."""
    g = gen(seed)
    M = generic(g, V, rows, L)
    x = (generic(g, rows, L).double() + offset).float()
    gamma = (torch.rand(G * (L // S), generator=g) + 0.5) * (torch.randint(0, 2, (G * (L // S),), generator=g) * 2 - 1).float() if affine else None
    return M, x, gamma


# ---- activations ----------------------------------------------------------------------------------------------------------------------
BETA, KAPPA = math.sqrt(2.0 / math.pi), 0.044715


def act_derivative(kind, x):
    """(f'(x), bound) in fp64 at the fp32 points ``x``.  The bounds follow the expressions of the kernel term by term, with OCML's
    documented accuracies (expf 1 ulp, tanhf 2 ulp, erff 4 ulp; 1 ulp <= 2 eps relative) and one eps per fp32 operation; FLT_MIN
    stands for results that leave the normal range (expf overflows to inf beyond 88.7, where the true derivative is below 1e-38).

    gelu: cdf = 0.5 (1 + erf(x / sqrt 2)): 4 ulp of erf near 1 = 8 eps, halved; the rounded argument moves erf by at most eps; two
      more operations: 6 eps absolute.  x pdf = x exp(-x^2 / 2) c: the exponent carries two roundings (x^2 eps relative on exp), exp 2 eps,
      three products: (x^2 + 5) eps |x pdf|.  The final addition: eps (1 + |x pdf|).
    silu: s = 1 / (1 + exp(-x)): 4 eps relative.  1 - s: 4 eps s + eps (1 - s).  g = 1 + x (1 - s): |x| (4 s + 2 (1 - s)) eps + eps |g|.
      s g: 4 eps |s g| + s dg + eps |s g|.
    gelu_tanh: u = beta (x + kappa x^3): 4 eps |u|;  t = tanh u: dt = 4 eps |t| + (1 - t^2) 4 eps |u|;  0.5 (1 + t): 0.5 dt + eps;
      1 - t^2: 2 |t| dt + 2 eps;  du/dx = beta (1 + 3 kappa x^2): 4 eps relative;  the product 0.5 x (1 - t^2) du/dx: 7 eps relative on top;
      the final addition eps |result|."""
    x = x.to(F64)
    e = EPS
    if kind == "gelu":
        cdf = 0.5 * (1 + torch.erf(x / math.sqrt(2.0)))
        xp = x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
        return cdf + xp, e * (7 + (x * x + 6) * xp.abs()) + FLT_MIN
    if kind == "silu":
        s = torch.sigmoid(x)
        g = 1 + x * (1 - s)
        dg = x.abs() * (4 * s + 2 * (1 - s)) * e + e * g.abs()
        return s * g, 5 * e * (s * g).abs() + s * dg + FLT_MIN
    u = BETA * (x + KAPPA * x ** 3)
    t = torch.tanh(u)
    dudx = BETA * (1 + 3 * KAPPA * x * x)
    right = 0.5 * x * (1 - t * t) * dudx
    res = 0.5 * (1 + t) + right
    dt = 4 * e * t.abs() + (1 - t * t) * 4 * e * u.abs()
    bound = 0.5 * dt + e + (0.5 * x * dudx).abs() * (2 * t.abs() * dt + 2 * e) + 7 * e * right.abs() + e * res.abs() + FLT_MIN
    return res, bound


def act_module(kind):
    from torch import nn

    return {"gelu": nn.GELU(), "gelu_tanh": nn.GELU(approximate="tanh"), "silu": nn.SiLU()}[kind]
