"""fp64 reference and derived error bounds for the cross-attention rule (csrc/attention.hip, ``vivit_attention_cross_jac_t_f32``).
TEST INFRASTRUCTURE shared by tests/test_attention_cross_refs_host.py, tests/test_attention_cross_rule_gpu.py and
tests/test_attention_cross_layers.py; it builds on tests/attention_masked_refs.py (constants, helpers, the form of the bounds) and
tests/attention_gqa_refs.py (the head layout), and edits neither.

Layout.  ``q [N, Tq, H d]``, ``kv [N, Tk, 2 Hkv d]`` = k | v (``Hkv`` key heads, then ``Hkv`` value heads), ``M`` and
``out [.., N, Tq, H d]``; ``Gq [V, N, Tq, H d]`` = dQ and ``Gkv [V, N, Tk, 2 Hkv d]`` = dK | dV.  Query head ``h`` uses key / value head
``h // R``, ``R = H / Hkv``.

The mask.  No causal flag and no window.  Sample ``n`` has ``Lq_n`` queries and ``Lk_n`` keys (``Tq`` / ``Tk`` without lengths; right
padding, clamped to ``[0, Tq]`` / ``[0, Tk]``).  Key ``j`` is live iff ``j < Lk_n``; query ``i`` is live iff ``i < Lq_n`` and ``Lk_n > 0``.
A live query sees every live key.  Dead positions: the reference replaces their data by zeros before anything else (NaN there changes
nothing), gives a dead query key 0 to look at so that its row of the softmax is finite (on its zeroed data every quantity of the row
is 0), and then SETS the rows of the dead positions of both results: reference 0, bound 2^-126 -- only an exact zero passes.

Error bounds: those of ``attention_masked_refs.rule`` with the lengths of the sums replaced.  A row of S has ``Tk`` entries, so the
terms of lse and dQ that count the summands of a row take ``Tk`` for ``T`` and ``KB = ceil(Tk / 32)`` key blocks for the rescalings of
the running sum; dK and dV are dot products over the ``R Tq`` pairs (head, query) of the group, so their terms take ``R Tq`` for
``R T``.  Everything else (S, P, D, dP, dS: per entry, contraction length ``d``) is unchanged.
"""
import math

import torch

import attention_masked_refs as mr
from attention_masked_refs import BLOCK, D_MAX, EPS, F64, FLT_MIN, chunk, gen, misaligned, within   # noqa: F401  (re-exported)

gr = mr.gr
HEADS = [(2, None), (3, 3), (4, 2), (4, 1), (6, 3)]   # (H, Hkv): no num_kv_heads, R = 1, 2, 4, 2
DIMS = [1, 16, 17, 32, 33, 64, 65, 128]              # the smallest and the largest d of each instance of the kernel
SHAPES = [(1, 1), (1, 33), (5, 97), (32, 32), (33, 32), (32, 33), (65, 5), (64, 65), (97, 161), (161, 97)]   # (Tq, Tk)
LENGTHS = (0, 1, 31, 32, 33, 64, 65)                 # and T itself: what a case draws its lengths from (those that fit)

# (Tq, Tk, query lengths, key lengths); N is the number of lengths (2 without any)
_SPEC = [
    (1, 1, None, None),                                      # no lengths
    (1, 33, (1, 0), (33, 31)),
    (5, 97, (5, 1, 0), (97, 65, 33)),
    (32, 32, None, (32, 1, 31)),                             # only key lengths
    (33, 32, (33, 32, 1), (32, 31, 0)),                      # Lk = 0 beside live queries
    (32, 33, (0, 0, 0), (0, 0, 0)),                          # every length 0
    (65, 5, (65, 64, 33, 0), (5, 1, 5, 5)),
    (64, 65, (64, 31, 32), None),                            # only query lengths
    (97, 161, (97, 65, 33, 1), (161, 64, 31, 0)),
    (161, 97, (161, 64, 32, 0), (97, 65, 1, 33)),
    (97, 161, None, None),
    (161, 97, (33, 161, 65), (97, 0, 32)),
    (33, 32, None, (0, 32)),                                 # Lk = 0 beside live queries, no query lengths
    (5, 97, (5, 5), (97, 97)),                               # every length T
    (64, 65, (64, 1, 0, 32), (65, 64, 33, 1)),
    (65, 5, None, None),
    (32, 33, (31, 32, 1), (33, 32, 31)),
    (1, 33, (1, 1, 1), (0, 1, 32)),
    (32, 32, (32, 0), (31, 32)),
    (1, 1, (1, 0, 1), (1, 1, 0)),
    (161, 97, None, (65, 97, 64)),
    (97, 161, (64, 97), (1, 161)),
    (33, 32, (33, 33), (32, 32)),
    (65, 5, (1, 65, 31), (5, 0, 1)),
]


def _cases():
    """(Tq, Tk, d, H, Hkv, V, N, scale, query lengths, key lengths); ``Hkv`` None: the call without ``num_kv_heads``."""
    cases = []
    for k, (Tq, Tk, ql, kl) in enumerate(_SPEC):
        d, (H, Hkv) = DIMS[k % 8], HEADS[k % 5]
        c = chunk(d)
        V = c - 1 if (k // 8 + k) % 2 == 0 else 2 * c + 1     # (k and k + 8 share d and differ here)
        N = len(ql) if ql is not None else len(kl) if kl is not None else 2
        cases.append((Tq, Tk, d, H, Hkv, V, N, -0.5 if k == 7 else None, ql, kl))
    return cases


# The cases of tests/test_attention_cross_rule_gpu.py (shared with the host test, which checks this rule).  The rule of the list: every
# instance of the kernel (d <= 16, <= 32, <= 64, <= 128) meets its smallest d (never a multiple of four) and its largest, each with a V of
# one chunk minus one and of two chunks plus one; (H, Hkv) as HEADS; every (Tq, Tk) of SHAPES at least twice -- both sequences on, one
# past and one short of a block edge, each longer than the other by several blocks; lengths from {0, 1, 31, 32, 33, 64, 65, T}, drawn
# independently for the two sides and mixed within a batch; cases with no lengths, with key lengths only, with query lengths only, with
# Lk = 0 beside live queries, with every length 0 and with every length T; one negative scale.  Nothing is larger than
# Tq, Tk = 161, H = 6, d = 128, V = 9, N = 4.
CASES = _cases()
assert {(c[0], c[1]) for c in CASES} == set(SHAPES) and {c[2] for c in CASES} == set(DIMS) and {(c[3], c[4]) for c in CASES} == set(HEADS)
assert all({c[5] for c in CASES if c[2] == d} == {chunk(d) - 1, 2 * chunk(d) + 1} for d in DIMS)


def live_lengths(Tq, Tk, query_lengths, key_lengths, N):
    """Per sample ``(Lq, Lk)``: clamped, and ``Lq = 0`` where ``Lk = 0`` (a query with no key to look at is dead)."""
    both = []
    for n in range(N):
        Lk = Tk if key_lengths is None else min(max(int(key_lengths[n]), 0), Tk)
        Lq = Tq if query_lengths is None else min(max(int(query_lengths[n]), 0), Tq)
        both.append((Lq if Lk > 0 else 0, Lk))
    return both


def dead(Tq, Tk, query_lengths, key_lengths, N):
    """``(dead_q [N, Tq], dead_k [N, Tk])`` bool, written sample by sample from the definition."""
    dq, dk = torch.ones(N, Tq, dtype=torch.bool), torch.ones(N, Tk, dtype=torch.bool)
    for n, (Lq, Lk) in enumerate(live_lengths(Tq, Tk, query_lengths, key_lengths, N)):
        dq[n, :Lq] = False
        dk[n, :Lk] = False
    return dq, dk


def _hidden(dq, dk):
    """``[N, 1, 1, Tq, Tk]``: the pairs that do not see each other; a dead query keeps key 0 (see the docstring)."""
    vis = ~dq[:, :, None] & ~dk[:, None, :]
    vis[:, :, 0] |= dq
    return ~vis[:, None, None]


def split(q, kv, H, Hkv):
    """``q [*B, Tq, H d]``, ``kv [*B, Tk, 2 Hkv d]`` -> ``q [*B, Hkv, R, Tq, d]``, ``k`` and ``v [*B, Hkv, 1, Tk, d]``."""
    half = kv.shape[-1] // 2
    return gr.heads(q, Hkv, H // Hkv), gr.heads(kv[..., :half], Hkv, 1), gr.heads(kv[..., half:], Hkv, 1)


def forward(q, kv, H, Hkv, scale, query_lengths=None, key_lengths=None):
    """The module output in the dtype of ``q`` (``[N, Tq, H d]``), rows of zeros at the dead queries."""
    N, Tq, Tk = q.shape[0], q.shape[1], kv.shape[1]
    dq, dk = dead(Tq, Tk, query_lengths, key_lengths, N)
    qh, k, v = split(q.masked_fill(dq[:, :, None], 0.0), kv.masked_fill(dk[:, :, None], 0.0), H, Hkv)
    S = ((qh @ k.transpose(-1, -2)) * scale).masked_fill(_hidden(dq, dk), float("-inf"))
    return (S.softmax(-1) @ v).movedim(-2, 1).reshape(N, Tq, -1).masked_fill(dq[:, :, None], 0.0)


def logits(q, kv, H, Hkv, scale):
    """S [N, Hkv, R, Tq, Tk] in fp64 (unmasked)."""
    qh, k, _ = split(q.to(F64), kv.to(F64), H, Hkv)
    return (qh @ k.transpose(-1, -2)) * scale


def rule(M, q, kv, out, H, Hkv, scale, query_lengths=None, key_lengths=None):
    """``M [V, N, Tq, H d]``, ``q [N, Tq, H d]``, ``kv [N, Tk, 2 Hkv d]``, ``out [N, Tq, H d]`` -> ``(Gq, bound of Gq, Gkv, bound of
    Gkv)``, the results in fp64 and their elementwise bounds."""
    V, N, Tq, E = M.shape
    Tk, d, R = kv.shape[1], E // H, H // Hkv
    dq, dk = dead(Tq, Tk, query_lengths, key_lengths, N)
    dq3, dk3 = dq[:, :, None], dk[:, :, None]
    qh, k, v = split(q.to(F64).masked_fill(dq3, 0.0), kv.to(F64).masked_fill(dk3, 0.0), H, Hkv)
    dO, O = gr.heads(M.to(F64).masked_fill(dq3, 0.0), Hkv, R), gr.heads(out.to(F64).masked_fill(dq3, 0.0), Hkv, R)
    a = abs(scale)
    mask = _hidden(dq, dk)
    S = ((qh @ k.transpose(-1, -2)) * scale).masked_fill(mask, float("-inf"))
    e_S = ((d + 3) * EPS * a * (qh.abs() @ k.abs().transpose(-1, -2))).masked_fill(mask, 0.0)
    lse = torch.logsumexp(S, -1, keepdim=True)
    arg = (S - lse).masked_fill(mask, 0.0)
    P = torch.exp(S - lse)
    KB, lnT = math.ceil(Tk / BLOCK), math.log(max(Tk, 2))
    e_lse = e_S.amax(-1, keepdim=True) + EPS * (lse.abs() + Tk + 4 + KB * (lnT + 5) + 3 * lnT)
    e_P = (P * (e_S + e_lse + EPS * (arg.abs() + 2)) + FLT_MIN).masked_fill(mask, 0.0)
    D = (dO * O).sum(-1, keepdim=True)
    e_D = (d + 1) * EPS * (dO * O).abs().sum(-1, keepdim=True)
    dP = dO @ v.transpose(-1, -2)
    e_dP = (d + 2) * EPS * (dO.abs() @ v.abs().transpose(-1, -2))
    W = dP - D
    dS = P * W
    e_dS = e_P * W.abs() + P * (e_dP + e_D) + 2 * EPS * dS.abs()
    dQ = (dS @ k) * scale
    e_dQ = a * (e_dS @ k.abs() + (Tk + 3) * EPS * (dS.abs() @ k.abs()))
    Pt, dSt = P.transpose(-1, -2), dS.transpose(-1, -2)
    dV = (Pt @ dO).sum(3)
    e_dV = (e_P.transpose(-1, -2) @ dO.abs()).sum(3) + (R * Tq + 2) * EPS * (Pt @ dO.abs()).sum(3)
    dK = (dSt @ qh).sum(3) * scale
    e_dK = a * ((e_dS.transpose(-1, -2) @ qh.abs()).sum(3) + (R * Tq + 3) * EPS * (dSt.abs() @ qh.abs()).sum(3))
    rows = lambda t, T: t.movedim(-2, 2).reshape(V, N, T, -1)   # noqa: E731  ([V, N, heads.., T, d] -> [V, N, T, heads d])
    Gq, bq = rows(dQ, Tq), rows(e_dQ, Tq) + FLT_MIN
    Gkv, bkv = torch.cat((rows(dK, Tk), rows(dV, Tk)), -1), torch.cat((rows(e_dK, Tk), rows(e_dV, Tk)), -1) + FLT_MIN
    return Gq.masked_fill(dq3, 0.0), bq.masked_fill(dq3, FLT_MIN), Gkv.masked_fill(dk3, 0.0), bkv.masked_fill(dk3, FLT_MIN)


def make_case(seed, V, N, Tq, Tk, H, Hkv, d, scale=None, query_lengths=None, key_lengths=None, qk_gain=1.0):
    """Seeded fp32 operands (CPU): ``(M, q, kv, out, scale)``; the data of the dead positions is ordinary (finite) data, ``out`` is
    the masked forward pass (zero rows at the dead queries); ``qk_gain`` multiplies q and k (large logits)."""
    g = gen(seed)
    E = H * d
    q = torch.randn(N, Tq, E, generator=g) * qk_gain
    kv = torch.randn(N, Tk, 2 * Hkv * d, generator=g)
    kv[..., :Hkv * d] *= qk_gain
    M = torch.randn(V, N, Tq, E, generator=g) * 10.0 ** (torch.rand(V, N, Tq, E, generator=g) * 2 - 1)
    scale = d ** -0.5 if scale is None else scale
    return M, q, kv, forward(q, kv, H, Hkv, scale, query_lengths, key_lengths), scale


_OPERANDS = {}


def case_operands(case):
    """``(M, q, kv, out, scale, Hkv_eff)`` of a case of the list (``Hkv_eff = H`` without ``num_kv_heads``); computed once per case
    and shared: callers leave the tensors unchanged."""
    if case not in _OPERANDS:
        Tq, Tk, d, H, Hkv, V, N, scale, ql, kl = case
        He = H if Hkv is None else Hkv
        _OPERANDS[case] = make_case(1000 * Tq + 7 * Tk + d + H, V, N, Tq, Tk, H, He, d, scale, ql, kl) + (He,)
    return _OPERANDS[case]


_RULES = {}


def case_rule(case):
    """``rule`` of a case's operands, computed once per case and shared."""
    if case not in _RULES:
        M, q, kv, out, scale, He = case_operands(case)
        _RULES[case] = rule(M, q, kv, out, case[3], He, scale, case[8], case[9])
    return _RULES[case]
