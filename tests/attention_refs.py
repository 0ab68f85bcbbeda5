"""fp64 reference and derived error bounds for the attention rule (csrc/attention.hip, ``vivit_attention_jac_t_f32``).  TEST
INFRASTRUCTURE shared by tests/test_attention_rule_gpu.py and tests/test_attention_refs_host.py; in the manner of tests/norm_refs.py.

The reference restates the formula of include/vivit_hip.h in torch fp64 from the fp32 operands the kernel is given (the factor ``M``,
the packed projection ``qkv`` and the module output ``out``: an fp32 INPUT of the rule, used as it is).

Error bounds (eps = 2^-24, elementwise against the fp64 reference, first order in eps; derived, not fitted).  A dot product of length
L of fp32 numbers, in ANY order of summation and with or without fused multiply-adds, has the error (L + 2) eps sum|a_k b_k| at most
(one rounding per product, at most L - 1 additions on a path, one to spare): the convention of tests/epilogue_refs.py.  |X| is X with
absolute values taken elementwise, and every magnitude below is evaluated in fp64.

* S = scale Q K^T: length d and one more product, e_S = (d + 3) eps |scale| (|Q| |K|^T).
* lse_i = log sum_j exp(S_ij).  The map S_i -> lse_i moves by at most max_j |dS_ij|, so the error of S contributes max_j e_S,ij
  (over the unmasked j).  The kernel's own arithmetic: l = sum_j exp(S_ij - m), block after block with the running maximum m.  An
  argument S_ij - m is rounded once, which changes its term by the factor eps |S_ij - m|; weighted by the term's share of l these add
  up to eps sum_j p_j (m - S_ij) <= eps ln T.  expf is good to 1 ulp <= 2 eps; the sum has T terms ((T + 2) eps); at each of the KB =
  ceil(T / 32) blocks l is rescaled by exp(m_old - m_new), whose rounded argument changes l by at most eps (ln T + 1) relative (the
  maximum of D y / (y + 1) over y = l_old exp(-D) <= T exp(-D)), plus 2 eps for the expf and 2 for the product and the sum.  Then
  lse = m + log l with 0 <= log l <= ln T: logf 2 eps ln T, the addition eps |lse|.  Together
      e_lse = max_j e_S,ij + eps (|lse| + T + 4 + KB (ln T + 5) + 3 ln T).
* P = exp(S - lse): the argument carries e_S + e_lse and the rounding eps |S - lse| of the subtraction, expf adds 2 eps relative:
      e_P = P (e_S + e_lse + eps (|S - lse| + 2)) + 2^-126.
  This is the amplification through exp: with logits of +-200 and d = 20, e_S alone is 1e-4, a relative error of P that no later
  step removes.  2^-126 stands for results that leave the normal range (the true value of exp(-200) is 1e-87, fp32 gives 0).  Masked
  entries are exactly 0 on both sides.
* D_i = sum_c dO_ic O_ic, a serial fused chain: e_D = (d + 1) eps sum_c |dO_ic O_ic|.
* dP = dO V^T: e_dP = (d + 2) eps (|dO| |V|^T).
* dS = P o (dP - D): e_dS = e_P |dP - D| + P (e_dP + e_D) + 2 eps |dS|  (the subtraction and the product).
* dV = P^T dO, length T: e_dV = e_P^T |dO| + (T + 2) eps (P^T |dO|).
* dQ = scale dS K and dK = scale dS^T Q, length T and one more product:
      e_dQ = |scale| (e_dS |K| + (T + 3) eps (|dS| |K|)),   e_dK = |scale| (e_dS^T |Q| + (T + 3) eps (|dS|^T |Q|)).
Every final bound gets 2^-126 for results below the normal range.
"""
import math

import torch

from epilogue_refs import EPS, F64, gen, misaligned, within   # noqa: F401  (re-exported for the test modules)

FLT_MIN = 2.0 ** -126
BLOCK = 32        # queries per query block = keys per key block (ATT_B of csrc/attention.hip)
D_MAX = 128       # largest head dimension the kernel takes
TB = 2 * BLOCK + 1   # both owners walk three blocks, the last one ragged


def chunk(d):
    """Factor rows a workgroup takes at a time (AttCfg<NT>::VC of csrc/attention.hip)."""
    return 2 if d > 32 else 4


# The cases of tests/test_attention_rule_gpu.py (shared with tests/test_attention_refs_host.py), (T, d, H, V, N, causal, scale).
# The kernel has four instances (d <= 16, <= 32, <= 64, <= 128) and takes chunk(d) factor rows per workgroup.  The rule of the list:
# every instance meets a V of zero, one and two full chunks plus a remainder (and full chunks without one), every instance meets
# its smallest and its largest d, and T is listed both as exact multiples of 32 (32, 64) and as ragged lengths (1, 5, 16, 17, 33,
# TB = 65); H in {1, 2, 3}, N in {1, 2}, both masks; a negative and a zero scale once each.
CASES = [(1, 1, 1, 1, 1, False, None), (1, 4, 3, 3, 2, True, None), (1, 128, 1, 3, 1, False, None),
         (5, 20, 3, 1, 2, True, None), (5, 64, 1, 3, 1, False, None),
         (16, 4, 1, 3, 2, False, None), (16, 128, 3, 1, 1, True, None),
         (17, 1, 3, 3, 2, True, None), (17, 64, 1, 1, 2, False, 0.37), (17, 20, 3, 3, 1, False, None),
         (33, 20, 1, 3, 1, False, None), (33, 128, 3, 3, 2, True, None), (33, 4, 3, 1, 2, True, None),
         (TB, 4, 3, 1, 2, False, None), (TB, 64, 3, 3, 2, True, None), (TB, 128, 1, 3, 1, False, None), (TB, 20, 1, 3, 2, True, 0.5),
         (TB, 1, 1, 3, 1, True, None), (TB, 64, 1, 1, 1, False, None),
         # chunks of four rows (d <= 32): V = 4, 5, 8, 9
         (5, 1, 1, 4, 1, False, None), (33, 4, 1, 5, 1, True, None), (32, 16, 2, 5, 2, True, None), (17, 16, 2, 8, 1, False, None),
         (TB, 20, 1, 9, 2, True, None), (32, 32, 3, 8, 1, False, None), (33, 16, 1, 9, 1, True, None), (17, 32, 1, 6, 2, False, None),
         # chunks of two rows (d > 32): V = 4, 5
         (33, 64, 1, 4, 1, False, None), (17, 128, 1, 5, 1, True, None), (TB, 33, 2, 4, 1, True, None), (17, 64, 2, 5, 1, True, None),
         # the edges of the instances, and sequences that are whole blocks
         (64, 17, 1, 9, 1, False, None), (64, 32, 1, 3, 1, True, None), (33, 65, 1, 5, 2, False, -0.5), (64, 127, 1, 2, 1, True, None),
         (TB, 128, 1, 5, 1, True, None), (32, 33, 1, 1, 1, False, None),
         # scale 0: P is uniform over the unmasked keys, dQ and dK are exactly zero
         (33, 20, 2, 5, 1, True, 0.0)]


def forward(qkv, H, scale, causal):
    """The module output in the dtype of ``qkv`` (``[N, T, 3 E] -> [N, T, E]``)."""
    N, T, E3 = qkv.shape
    d = E3 // (3 * H)
    q, k, v = qkv.view(N, T, 3, H, d).permute(2, 0, 3, 1, 4)
    S = (q @ k.transpose(-1, -2)) * scale
    if causal:
        S = S.masked_fill(torch.ones(T, T, dtype=torch.bool).triu(1), float("-inf"))
    return (S.softmax(-1) @ v).transpose(1, 2).reshape(N, T, H * d)


def logits(qkv, H, scale):
    """S [N, H, T, T] in fp64 (unmasked)."""
    N, T, E3 = qkv.shape
    d = E3 // (3 * H)
    q, k, _ = qkv.to(F64).view(N, T, 3, H, d).permute(2, 0, 3, 1, 4)
    return (q @ k.transpose(-1, -2)) * scale


def rule(M, qkv, out, H, scale, causal):
    """``M [V, N, T, E]``, ``qkv [N, T, 3 E]``, ``out [N, T, E]`` -> (``G [V, N, T, 3 E]`` in fp64, its elementwise bound)."""
    V, N, T, E = M.shape
    d = E // H
    q, k, v = qkv.to(F64).view(N, T, 3, H, d).permute(2, 0, 3, 1, 4)       # each [N, H, T, d]
    dO = M.to(F64).view(V, N, T, H, d).permute(0, 1, 3, 2, 4)               # [V, N, H, T, d]
    O = out.to(F64).view(N, T, H, d).permute(0, 2, 1, 3)
    a = abs(scale)
    mask = torch.ones(T, T, dtype=torch.bool).triu(1) if causal else torch.zeros(T, T, dtype=torch.bool)
    S = ((q @ k.transpose(-1, -2)) * scale).masked_fill(mask, float("-inf"))
    e_S = ((d + 3) * EPS * a * (q.abs() @ k.abs().transpose(-1, -2))).masked_fill(mask, 0.0)
    lse = torch.logsumexp(S, -1, keepdim=True)
    arg = (S - lse).masked_fill(mask, 0.0)
    P = torch.exp(S - lse)
    KB, lnT = math.ceil(T / BLOCK), math.log(max(T, 2))
    e_lse = e_S.amax(-1, keepdim=True) + EPS * (lse.abs() + T + 4 + KB * (lnT + 5) + 3 * lnT)
    e_P = (P * (e_S + e_lse + EPS * (arg.abs() + 2)) + FLT_MIN).masked_fill(mask, 0.0)
    D = (dO * O).sum(-1, keepdim=True)
    e_D = (d + 1) * EPS * (dO * O).abs().sum(-1, keepdim=True)
    dP = dO @ v.transpose(-1, -2)
    e_dP = (d + 2) * EPS * (dO.abs() @ v.abs().transpose(-1, -2))
    W = dP - D
    dS = P * W
    e_dS = e_P * W.abs() + P * (e_dP + e_D) + 2 * EPS * dS.abs()
    dV = P.transpose(-1, -2) @ dO
    e_dV = e_P.transpose(-1, -2) @ dO.abs() + (T + 2) * EPS * (P.transpose(-1, -2) @ dO.abs())
    dQ = (dS @ k) * scale
    e_dQ = a * (e_dS @ k.abs() + (T + 3) * EPS * (dS.abs() @ k.abs()))
    dK = (dS.transpose(-1, -2) @ q) * scale
    e_dK = a * (e_dS.transpose(-1, -2) @ q.abs() + (T + 3) * EPS * (dS.abs().transpose(-1, -2) @ q.abs()))

    def pack(tq, tk, tv):
        return torch.stack((tq, tk, tv), 0).permute(1, 2, 4, 0, 3, 5).reshape(V, N, T, 3 * E)

    return pack(dQ, dK, dV), pack(e_dQ, e_dK, e_dV) + FLT_MIN


def make_case(seed, V, N, T, H, d, scale=None, causal=False, qk_gain=1.0):
    """Seeded fp32 operands (CPU): ``(M, qkv, out, scale)``; ``qk_gain`` multiplies q and k (large logits)."""
    g = gen(seed)
    E = H * d
    qkv = torch.randn(N, T, 3 * E, generator=g)
    qkv[..., :2 * E] *= qk_gain
    M = torch.randn(V, N, T, E, generator=g) * 10.0 ** (torch.rand(V, N, T, E, generator=g) * 2 - 1)
    scale = d ** -0.5 if scale is None else scale
    return M, qkv, forward(qkv, H, scale, causal), scale
