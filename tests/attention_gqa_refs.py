"""fp64 reference and derived error bounds for the grouped-query attention rule (csrc/attention.hip,
``vivit_attention_gqa_jac_t_f32``) and the rotary rule on its layout (``vivit_rope_gqa_jac_t_f32``).  TEST INFRASTRUCTURE shared by
tests/test_attention_gqa_refs_host.py, tests/test_attention_gqa_rule_gpu.py and tests/test_rope_gqa_gpu.py; it builds on
tests/attention_refs.py (whose conventions, constants and derivation it uses) and tests/llama_refs.py.

Layout: ``qkv [N, T, (H + 2 Hkv) d]`` = q (``H d`` columns) | k (``Hkv d``) | v (``Hkv d``); query head ``h`` attends to key / value
head ``g = h // R``, ``R = H / Hkv``.  ``M`` and ``out [.., N, T, H d]``; ``G [V, N, T, (H + 2 Hkv) d]`` = dQ | dK | dV.  Per query
head the formulas are those of tests/attention_refs.py with ``K_g``, ``V_g`` as operands, and
    dV_g = sum_{h in g} P_h^T dO_h,     dK_g = scale sum_{h in g} dS_h^T Q_h.

Error bounds: S, lse, P, D, dP, dS and dQ are per query head and keep the bounds of tests/attention_refs.py.  dV_g and dK_g are dot
products over the R T pairs (head, query) of the group, in whatever order -- the kernel's is head, then query block, then k within the
block -- so the (L + 2) eps convention applies with L = R T (and one more product for the scale of dK):
    e_dV_g = sum_{h in g} e_P,h^T |dO_h| + (R T + 2) eps sum_{h in g} P_h^T |dO_h|
    e_dK_g = |scale| (sum_{h in g} e_dS,h^T |Q_h| + (R T + 3) eps sum_{h in g} |dS_h|^T |Q_h|)
Every final bound gets 2^-126.  With Hkv == H (R = 1) reference and bounds are those of ``attention_refs.rule``.
"""
import math

import torch

import attention_refs as ar
import llama_refs as lr
from attention_refs import BLOCK, D_MAX, EPS, F64, FLT_MIN, TB, chunk, gen, misaligned, within   # noqa: F401  (re-exported)

INSTANCES = [(1, 16), (17, 32), (33, 64), (65, 128)]   # the head dimensions of the kernel's four instances


def _instance_cases(lo, hi, scales):
    """Six cases of one instance, (T, d, H, Hkv, V, N, causal, scale): see the rule below."""
    c = chunk(lo)
    s = scales + [None] * (6 - len(scales))
    return [(1, lo, 2, 1, c - 1, 1, False, s[0]), (5, hi, 6, 3, c, 2, True, s[1]), (32, lo, 3, 1, 2 * c + 1, 1, True, s[2]),
            (33, hi, 4, 2, c - 1, 2, False, s[3]), (TB, hi, 4, 1, 2 * c + 1, 1, True, s[4]), (TB, lo, 6, 2, c, 2, False, s[5])]


# The cases of tests/test_attention_gqa_rule_gpu.py (shared with the host test).  The rule of the list: every instance of the kernel
# (d <= 16, <= 32, <= 64, <= 128) meets its smallest d (never a multiple of four: the scalar load body at the unaligned k and v
# offsets) and its largest; R in {2, 3, 4} and Hkv in {1, 2, 3}; a V of one chunk minus one, one chunk, and two chunks plus one;
# T in {1, 5, 32, 33, 65} (65: three blocks with a ragged last one, so the owner's walk crosses head boundaries on full and on ragged
# blocks); both masks and N in {1, 2}.  One negative and one zero scale.  Nothing is larger than T = 65, H = 6, d = 128, V = 9, N = 2.
CASES = (_instance_cases(1, 16, [None, 0.0]) + _instance_cases(17, 32, [None, None, None, -0.5]) + _instance_cases(33, 64, [None, 0.37])
         + _instance_cases(65, 128, []) + [(TB, 128, 6, 3, 5, 2, True, None)])


def split(x, H, Hkv):
    """``x [*B, T, (H + 2 Hkv) d]`` -> ``q [*B, Hkv, R, T, d]``, ``k`` and ``v [*B, Hkv, 1, T, d]``."""
    d = x.shape[-1] // (H + 2 * Hkv)
    R, T, B = H // Hkv, x.shape[-2], x.shape[:-2]
    q = x[..., :H * d].reshape(*B, T, Hkv, R, d).movedim(-4, -2)
    k = x[..., H * d:(H + Hkv) * d].reshape(*B, T, Hkv, 1, d).movedim(-4, -2)
    v = x[..., (H + Hkv) * d:].reshape(*B, T, Hkv, 1, d).movedim(-4, -2)
    return q, k, v


def heads(x, Hkv, R):
    """``x [*B, T, H d]`` (the module output or the factor) -> ``[*B, Hkv, R, T, d]``."""
    return x.reshape(*x.shape[:-1], Hkv, R, -1).movedim(-4, -2)


def forward(qkv, H, Hkv, scale, causal):
    """The module output in the dtype of ``qkv`` (``[N, T, (H + 2 Hkv) d] -> [N, T, H d]``)."""
    N, T, _ = qkv.shape
    q, k, v = split(qkv, H, Hkv)
    S = (q @ k.transpose(-1, -2)) * scale
    if causal:
        S = S.masked_fill(torch.ones(T, T, dtype=torch.bool).triu(1), float("-inf"))
    return (S.softmax(-1) @ v).movedim(-2, 1).reshape(N, T, -1)


def logits(qkv, H, Hkv, scale):
    """S [N, Hkv, R, T, T] in fp64 (unmasked)."""
    q, k, _ = split(qkv.to(F64), H, Hkv)
    return (q @ k.transpose(-1, -2)) * scale


def pack(dQ, dK, dV):
    """``dQ [V, N, Hkv, R, T, d]``, ``dK`` and ``dV [V, N, Hkv, T, d]`` -> ``[V, N, T, (H + 2 Hkv) d]``."""
    V, N, _, _, T, _ = dQ.shape
    return torch.cat((dQ.movedim(-2, 2).reshape(V, N, T, -1), dK.movedim(-2, 2).reshape(V, N, T, -1),
                      dV.movedim(-2, 2).reshape(V, N, T, -1)), -1)


def rule(M, qkv, out, H, Hkv, scale, causal):
    """``M [V, N, T, H d]``, ``qkv [N, T, (H + 2 Hkv) d]``, ``out [N, T, H d]`` -> (``G`` in fp64, its elementwise bound)."""
    V, N, T, E = M.shape
    d, R = E // H, H // Hkv
    q, k, v = split(qkv.to(F64), H, Hkv)                                   # [N, Hkv, R | 1, T, d]
    dO, O = heads(M.to(F64), Hkv, R), heads(out.to(F64), Hkv, R)           # [V, N, Hkv, R, T, d], [N, Hkv, R, T, d]
    a = abs(scale)
    mask = torch.ones(T, T, dtype=torch.bool).triu(1) if causal else torch.zeros(T, T, dtype=torch.bool)
    # per query head, as tests/attention_refs.py
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
    dQ = (dS @ k) * scale
    e_dQ = a * (e_dS @ k.abs() + (T + 3) * EPS * (dS.abs() @ k.abs()))
    # per group: the sums over its R query heads (dimension 3 of [V, N, Hkv, R, T, d])
    Pt, dSt = P.transpose(-1, -2), dS.transpose(-1, -2)
    dV = (Pt @ dO).sum(3)
    e_dV = (e_P.transpose(-1, -2) @ dO.abs()).sum(3) + (R * T + 2) * EPS * (Pt @ dO.abs()).sum(3)
    dK = (dSt @ q).sum(3) * scale
    e_dK = a * ((e_dS.transpose(-1, -2) @ q.abs()).sum(3) + (R * T + 3) * EPS * (dSt.abs() @ q.abs()).sum(3))
    return pack(dQ, dK, dV), pack(e_dQ, e_dK, e_dV) + FLT_MIN


def make_case(seed, V, N, T, H, Hkv, d, scale=None, causal=False, qk_gain=1.0):
    """Seeded fp32 operands (CPU): ``(M, qkv, out, scale)``; ``qk_gain`` multiplies q and k (large logits)."""
    g = gen(seed)
    E = H * d
    qkv = torch.randn(N, T, (H + 2 * Hkv) * d, generator=g)
    qkv[..., :(H + Hkv) * d] *= qk_gain
    M = torch.randn(V, N, T, E, generator=g) * 10.0 ** (torch.rand(V, N, T, E, generator=g) * 2 - 1)
    scale = d ** -0.5 if scale is None else scale
    return M, qkv, forward(qkv, H, Hkv, scale, causal), scale


def expand(qkv, H, Hkv):
    """K and V repeated to ``H`` heads: the packed projection ``[N, T, 3 H d]`` of the multi-head module that computes the same."""
    d, R = qkv.shape[-1] // (H + 2 * Hkv), H // Hkv
    q, k, v = qkv[..., :H * d], qkv[..., H * d:(H + Hkv) * d], qkv[..., (H + Hkv) * d:]
    rep = lambda t: t.unflatten(-1, (Hkv, d)).repeat_interleave(R, -2).flatten(-2)   # noqa: E731
    return torch.cat((q, rep(k), rep(v)), -1)


# ---- rotary -------------------------------------------------------------------------------------------------------------------------
ROPE_HEADS = [(2, 1), (4, 2), (3, 1), (3, 3)]
ROPE_D = [2, 4, 6, 64, 128]
ROPE_T = [1, 33]
rope_tables = lr.rope_tables


def rope(M, cos, sin, H, Hkv, dtype=F64):
    """``M [R, T, (H + 2 Hkv) d]``, ``cos`` / ``sin [T, d / 2]`` -> (G like M, bound): the H + Hkv heads of the q and k parts rotated
    back under the bound of tests/llama_refs.py (2 eps (|m1 c| + |m2 s|) and 2 eps (|m2 c| + |m1 s|)), the v part as it is, bound 0."""
    R, T, W = M.shape
    d = W // (H + 2 * Hkv)
    half, rot_heads = d // 2, H + Hkv
    m = M.to(dtype)
    mr = m[..., :rot_heads * d].reshape(R, T, rot_heads, d)
    c, s = cos.to(dtype).view(1, T, 1, half), sin.to(dtype).view(1, T, 1, half)
    m1, m2 = mr[..., :half], mr[..., half:]
    rot = torch.cat((m1 * c + m2 * s, m2 * c - m1 * s), -1).reshape(R, T, rot_heads * d)
    mag = torch.cat(((m1 * c).abs() + (m2 * s).abs(), (m2 * c).abs() + (m1 * s).abs()), -1).reshape(R, T, rot_heads * d)
    tail = m[..., rot_heads * d:]
    return torch.cat((rot, tail), -1), torch.cat((2 * EPS * mag, torch.zeros_like(tail)), -1)
