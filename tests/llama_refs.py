"""fp64 references and derived error bounds for the RMSNorm, gated-product and rotary kernels (csrc/llama_rules.hip).  TEST
INFRASTRUCTURE shared by tests/test_llama_refs_host.py (no GPU) and tests/test_llama_kernels_gpu.py; in the manner of
tests/norm_refs.py.

Every reference restates the formula of include/vivit_hip.h in torch fp64.  The rules take ``rstd`` (and the rotary rule its tables)
as fp32 INPUTS, so their references use the very fp32 values the kernel was given; the statistics have a test of their own.

Error bounds (eps = 2^-24, elementwise against the fp64 reference, first order in eps; derived, not fitted):

* A sum of fp32 terms t_i along any fixed tree has the running-error bound  depth * eps * sum |t_i|, depth = the number of additions
  on the longest path from a term to the result.  The kernels sum a row of L elements as csrc/norm_rules.hip does: a serial sum per
  lane (T lanes; T = 64 on the wave route, L <= 1024, else 256), a butterfly over the 64 lanes of a wave (6 levels) and, on the
  workgroup route, the four wave sums one after the other (3).  :func:`sum_depth` counts exactly that.
* rstd = 1 / sqrt(sum(x^2) / L + e): the terms x^2 enter through fused multiply-adds (no rounding of their own) and are all
  positive, so the sum is depth eps RELATIVE; the division adds 1, the addition of e at most 1; the square root halves that and adds
  1, the reciprocal 1:   |d rstd| / rstd <= (0.5 (depth + 2) + 2) eps.
* xhat = x * rstd: one rounding.  h = gamma M: one rounding (none without gamma; the bound does not use that).
* c2 = sum(h xhat) / L: (depth + 3) eps mean|h xhat|  (h: 1, xhat: 1, the fused multiply-add counted in depth, the division: 1).
* out = rstd (h - xhat c2).  Term h: its rounding, the subtraction and the final product, 3 eps |rstd h|.  Term xhat c2: xhat 1, c2
  depth + 3, the product 1, the subtraction 1, the final product 1: (depth + 7) eps |rstd xhat| mean|h xhat|.  Together at most
      (depth + 7) eps |rstd| (|h| + |xhat| mean|h xhat|).
* w = M xhat: two roundings, 2 eps |M xhat|.
* position sums over A, serial fused multiply-adds: (A + 1) eps sum_a |M x rstd|  (xhat: 1, at most A additions).
* gate: a single rounded product each -- no bound, it must equal torch's fp32 product bit for bit.
* rotary: G1 = fmaf(m2, s, m1 c): the product m1 c is rounded (eps |m1 c|), the fused multiply-add once (eps |G1| <= eps (|m1 c| +
  |m2 s|)): 2 eps (|m1 c| + |m2 s|); G2 likewise with 2 eps (|m2 c| + |m1 s|).  The v third: bit for bit.
* rule(forward(x)) = x (a rotation's transpose is its inverse), with the fp32 tables c, s of the module: the forward pass y1 = x1 c - x2 s
  has 2 eps (|x1 c| + |x2 s|) <= 2 eps (|x1| + |x2|) max(|c|, |s|), which the rule multiplies by |c| + |s| <= sqrt 2 in all: 2 sqrt 2 eps
  (|x1| + |x2|); the rule's own 2 eps (|y1 c| + |y2 s|) <= 2 sqrt 2 eps (|x1| + |x2|); and c^2 + s^2 = 1 + delta with the tables within
  2 ulp = 4 eps of the true cosine and sine of one angle, |delta| <= 8 eps, on |x1|, while the cross terms x2 (c s - s c) cancel
  exactly.  In all (4 sqrt 2 + 8) eps < 14 eps (|x1| + |x2|).
"""
import math

import torch

from epilogue_refs import EPS, F64, gen, generic, misaligned, within   # noqa: F401  (re-exported for the test modules)

WAVE_L = 1024     # rows up to this length are held by one wavefront (RMS_WAVE_L of csrc/llama_rules.hip)
RMS_EPS = 1e-5

# ---- the cases of the GPU tests (shared with the host test) ---------------------------------------------------------------------
ROW_L = [1, 3, 64, 255, 256, 1024, 1027, 4100]       # both routes and the edge of each; both bodies
ROWS = [1, 5, 7]                                     # not multiples of the four rows per workgroup
VS = [1, 3]
POSITION_CASES = [(D, A, V) for D in (3, 256, 300) for A in (1, 5) for V in (1, 3)]
GATE_N = [1, 3, 4, 255, 256, 1025, 4100]
ROPE_D = [2, 4, 6, 64, 130]                          # d = 6: a half of odd length; 64: the 16-byte body; 130: odd half again
ROPE_CASES = [(d, T, H, R) for d in ROPE_D for (T, H, R) in ((1, 1, 1), (5, 3, 6), (33, 1, 6), (5, 3, 1))]


def sum_depth(L, vec):
    """Additions on the longest path of the kernels' sum over a row of ``L`` elements (``vec``: the 16-byte body)."""
    T = 64 if L <= WAVE_L else 256
    serial = 4 * math.ceil(L / (4 * T)) if vec else math.ceil(L / T)
    return serial + 6 + (3 if L > WAVE_L else 0)


# ---- RMSNorm ------------------------------------------------------------------------------------------------------------------------
def stats(x, eps):
    """x [rows, L] -> rstd in fp64."""
    return 1.0 / torch.sqrt((x.to(F64) ** 2).mean(1) + eps)


def stats_bound(x, eps, vec):
    return (0.5 * (sum_depth(x.shape[1], vec) + 2) + 2) * EPS * stats(x, eps)


def rules(M, x, gamma, rstd):
    """M [V, rows, L], x [rows, L], gamma [L] or None, rstd [rows] -> (out, w) and the magnitudes their bounds are made of."""
    M, x, rstd = M.to(F64), x.to(F64), rstd.to(F64)[:, None]
    h = M if gamma is None else gamma.to(F64) * M
    xhat = x * rstd
    out = rstd * (h - xhat * (h * xhat).mean(2, keepdim=True))
    w = M * xhat
    mag_out = rstd.abs() * (h.abs() + xhat.abs() * (h * xhat).abs().mean(2, keepdim=True))
    return (out, w), (mag_out, w.abs())


def rules_bounds(mags, L, vec):
    return (sum_depth(L, vec) + 7) * EPS * mags[0], 2 * EPS * mags[1]


def position_sums(M, x, rstd):
    """M [V, N, A, D], x [N, A, D], rstd [N A] -> pw [V, N, D] and its bound."""
    V, N, A, D = M.shape
    t = M.to(F64) * (x.to(F64) * rstd.to(F64).view(N, A, 1))
    return t.sum(2), (A + 1) * EPS * t.abs().sum(2)


def make_rows(seed, V, rows, L, affine=True):
    """Seeded operands (CPU fp32): M [V, rows, L], x [rows, L], gamma [L] with both signs, away from 1."""
    g = gen(seed)
    M, x = generic(g, V, rows, L), generic(g, rows, L)
    gamma = (torch.rand(L, generator=g) + 0.5) * (torch.randint(0, 2, (L,), generator=g) * 2 - 1).float() if affine else None
    return M, x, gamma


def fp32_stats(x, eps=RMS_EPS):
    """fp32 rstd for the rules tests: the fp64 statistic rounded (the rules take it as an input)."""
    return stats(x, eps).float()


# ---- rotary -------------------------------------------------------------------------------------------------------------------------
def rope_tables(T, d, base=10000.0):
    """fp32 tables [T, d / 2] as the module computes them (angles in fp32)."""
    j = torch.arange(d // 2, dtype=torch.float32)
    angle = torch.arange(T, dtype=torch.float32)[:, None] * (base ** (-2.0 * j / d))[None, :]
    return angle.cos(), angle.sin()


def rope(M, cos, sin, H, dtype=F64):
    """M [R, T, 3 H d], cos / sin [T, d / 2] -> (G like M, bound) with the q and k thirds rotated back and the v third as it is."""
    R, T, E3 = M.shape
    d = E3 // (3 * H)
    half = d // 2
    m = M.to(dtype).view(R, T, 3, H, d)
    c, s = cos.to(dtype).view(1, T, 1, 1, half), sin.to(dtype).view(1, T, 1, 1, half)
    m1, m2 = m[:, :, :2, :, :half], m[:, :, :2, :, half:]
    rot = torch.cat((m1 * c + m2 * s, m2 * c - m1 * s), -1)
    mag = torch.cat(((m1 * c).abs() + (m2 * s).abs(), (m2 * c).abs() + (m1 * s).abs()), -1)
    G = torch.cat((rot, m[:, :, 2:]), 2).reshape(R, T, E3)
    bound = torch.cat((2 * EPS * mag, torch.zeros_like(m[:, :, 2:])), 2).reshape(R, T, E3)
    return G, bound


def rope_forward(x, cos, sin, H, dtype=F64):
    """The rotation itself (the module's forward pass) on x [R, T, 3 H d]."""
    return rope(x, cos, -sin, H, dtype)[0]


def rope_roundtrip_bound(x, H):
    """14 eps (|x1| + |x2|) on the q and k thirds, 0 on v."""
    R, T, E3 = x.shape
    d = E3 // (3 * H)
    half = d // 2
    a = x.to(F64).abs().view(R, T, 3, H, d)
    pair = a[:, :, :2, :, :half] + a[:, :, :2, :, half:]
    return torch.cat((14 * EPS * torch.cat((pair, pair), -1), torch.zeros_like(a[:, :, 2:])), 2).reshape(R, T, E3)


# ---- guarded outputs ------------------------------------------------------------------------------------------------------------------
GUARD, GUARD_WORDS = -24601.0, 64    # (64 floats: the view keeps the 16-byte alignment of the buffer)


def guarded(shape, device, shift=False):
    """(buffer, contiguous view of ``shape`` pre-filled with NaN between guard words); ``shift``: the view 4 bytes off 16-byte
    alignment."""
    numel = math.prod(shape)
    off = GUARD_WORDS + (1 if shift else 0)
    buf = torch.full((numel + 2 * GUARD_WORDS + 1,), GUARD, dtype=torch.float32, device=device)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + numel].view(shape)
    view.fill_(float("nan"))
    return buf, view


def guards_intact(buf, view, shift=False):
    off = GUARD_WORDS + (1 if shift else 0)
    return bool((buf[:off] == GUARD).all()) and bool((buf[off + view.numel():] == GUARD).all())
