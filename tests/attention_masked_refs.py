"""fp64 reference and derived error bounds for the attention rule with per-sample sequence lengths and a sliding window
(csrc/attention.hip, ``vivit_attention_masked_jac_t_f32``).  TEST INFRASTRUCTURE shared by tests/test_attention_masked_refs_host.py,
tests/test_attention_masked_rule_gpu.py and tests/test_attention_masked_layers.py; it builds on tests/attention_gqa_refs.py (layout,
helpers, constants) and tests/attention_refs.py (the derivation of the bounds), and edits neither.

The mask.  Sample ``n`` has ``L_n`` positions (``lengths[n]``, ``T`` without lengths; right padding).  Query ``i`` sees key ``j`` iff
``i < L_n`` and ``j < L_n``, ``j <= i`` when ``causal``, and ``|i - j| < W`` when a window ``W >= 1`` is given (with ``causal``: the
``W`` keys ``i - W + 1 .. i``).  The positions ``t >= L_n`` are dead: invisible as keys, a zero output row as queries, rows of exact
zeros in ``G``, and their data is not used -- the reference replaces it by zeros before anything else, so NaN there changes nothing.

Reference: the formulas of tests/attention_gqa_refs.py with this mask in the place of the causal one (masked logits are ``-inf``,
masked entries of P, e_S and e_P exactly zero).  A dead query is given its own position to look at, which keeps its row of the softmax
finite (on zeroed data every quantity of the row is 0); the rows of the dead positions are then SET: reference 0, bound 2^-126, so
only an exact zero (of either sign) passes.

Error bounds: those of tests/attention_gqa_refs.py, unchanged.  Their terms ``T`` (the length of a row's sums: lse, dQ), ``R T`` (dK,
dV) and ``KB = ceil(T / 32)`` (the rescalings of the running sum of lse) count the pairs and the blocks of the unmasked function.  The
masked kernel adds up a subset of those pairs and visits a subset of those blocks, so the terms over-count what it does and the
bounds remain upper bounds; the magnitudes they multiply are sums over the visible pairs only, because P and dS are zero elsewhere.
"""
import math

import torch

import attention_gqa_refs as gr
from attention_gqa_refs import BLOCK, D_MAX, EPS, F64, FLT_MIN, INSTANCES, chunk, gen, misaligned, within   # noqa: F401  (re-exported)

LENGTHS = (0, 1, 31, 32, 33, 64, 65)      # and T itself: what a case draws its lengths from
T_ALL = (1, 5, 32, 33, 65, 97, 161)
HEADS = [(2, None), (3, 3), (4, 2), (4, 1), (6, 3)]   # (H, Hkv): multi-head attention (no num_kv_heads), R = 1, 2, 4, 2
DIMS = [1, 16, 17, 32, 33, 64, 65, 128]              # the smallest (never a multiple of four) and the largest d of each instance


def _cases():
    """(T, d, H, Hkv, V, N, causal, scale, lengths, window); ``Hkv`` None: the multi-head call, ``lengths`` a tuple or None."""
    spec = []
    # the windows around the block size and twice it: a walk reaches floor((W + 30) / 32) blocks from the diagonal, which is 1, 1, 2
    # for W = 32, 33, 34 and 2, 2, 3 for W = 64, 65, 66 (33 and 65 are the last windows that stop at the START of a block).  On four and
    # six blocks with a ragged last one, so that a walk skips blocks at its start and at its end; the first sample is full
    for T, others in ((97, (65, 33)), (161, (64, 31))):
        for W in (32, 33, 34, 64, 65):
            for causal in (False, True):
                spec.append((T, W, causal, (T,) + others))
    spec += [(161, 66, False, (161, 65, 32)), (161, 66, True, (161, 65, 32))]
    # few positions and the smallest windows; all lengths T, all lengths 0, no lengths, no window
    spec += [(1, 1, False, (1, 0)), (1, 6, True, None), (5, 2, True, (5, 1, 0)), (5, 5, False, (5, 5)), (32, 31, False, (32, 31, 1)),
             (32, 1, True, (32, 0, 31)), (33, 32, True, (33, 32, 31, 1)), (33, 2, False, (0, 33, 32)), (33, 38, False, (33, 1)),
             (65, 31, True, (65, 64, 33, 0)), (65, 65, True, (65, 65)), (65, 2, False, None), (65, 1, False, (64, 65, 32)),
             (97, None, True, (97, 65, 33, 0)), (161, None, False, (161, 64, 31, 1)), (65, None, True, (0, 0, 0)),
             (33, None, False, (33, 33)), (161, None, True, (32, 64, 65, 161)), (97, 97, False, (97, 64)), (161, 166, True, None),
             (161, 31, False, (65, 161, 33)), (97, 2, True, (1, 97, 32))]
    cases = []
    for k, (T, W, causal, lengths) in enumerate(spec):
        d, (H, Hkv) = DIMS[k % 8], HEADS[k % 5]
        c = chunk(d)
        V = c - 1 if (k // 8 + k) % 2 == 0 else 2 * c + 1
        N = 2 if lengths is None else len(lengths)
        cases.append((T, d, H, Hkv, V, N, causal, -0.5 if k == 7 else None, lengths, W))
    return cases


# The cases of tests/test_attention_masked_rule_gpu.py (shared with the host test, which checks this rule).  The rule of the list:
# every instance of the kernel (d <= 16, <= 32, <= 64, <= 128) meets its smallest d (never a multiple of four) and its largest; the
# multi-head call and grouped queries with R in {1, 2, 4}; T in {1, 5, 32, 33, 65, 97, 161}; lengths from {0, 1, 31, 32, 33, 64, 65, T}
# mixed within a batch, cases with every length T, with no lengths and one with every length 0; the windows {1, 2, 31, 32, 33, 34, 64,
# 65, T, T + 5} and none, with and without the causal mask, and every one of 32, 33, 34, 64, 65 with both masks at T = 97 and at
# T = 161; a V of one chunk minus one and of two chunks plus one in every instance; one negative scale.  Nothing is larger than
# T = 161, H = 6, d = 128, V = 9, N = 4.
CASES = _cases()


def visible(T, lengths, causal, window):
    """``[N, T, T]`` bool (``[1, T, T]`` without lengths): query i sees key j.  Written entry by entry from the definition."""
    Ls = [T] if lengths is None else [min(max(int(l), 0), T) for l in lengths]
    vis = torch.zeros(len(Ls), T, T, dtype=torch.bool)
    for n, L in enumerate(Ls):
        for i in range(L):
            lo = 0 if window is None else max(0, i - window + 1)
            hi = i if causal else (L - 1 if window is None else min(L - 1, i + window - 1))
            vis[n, i, lo:hi + 1] = True
    return vis


def dead(T, lengths, N):
    """``[N, T]`` bool: the positions ``t >= L_n``."""
    if lengths is None:
        return torch.zeros(N, T, dtype=torch.bool)
    L = torch.as_tensor([min(max(int(l), 0), T) for l in lengths])
    return torch.arange(T)[None, :] >= L[:, None]


def _hidden(N, T, lengths, causal, window):
    """``[N, 1, 1, T, T]``: the pairs that do not see each other; a dead query keeps its own position (see the docstring)."""
    vis = visible(T, lengths, causal, window).expand(N, T, T) | torch.eye(T, dtype=torch.bool)
    return ~vis[:, None, None]


def forward(qkv, H, Hkv, scale, causal, lengths=None, window=None):
    """The module output in the dtype of ``qkv`` (``[N, T, (H + 2 Hkv) d] -> [N, T, H d]``), rows of zeros at the dead positions."""
    N, T, _ = qkv.shape
    dd = dead(T, lengths, N)
    q, k, v = gr.split(qkv.masked_fill(dd[:, :, None], 0.0), H, Hkv)
    S = ((q @ k.transpose(-1, -2)) * scale).masked_fill(_hidden(N, T, lengths, causal, window), float("-inf"))
    return (S.softmax(-1) @ v).movedim(-2, 1).reshape(N, T, -1).masked_fill(dd[:, :, None], 0.0)


def rule(M, qkv, out, H, Hkv, scale, causal, lengths=None, window=None):
    """``M [V, N, T, H d]``, ``qkv [N, T, (H + 2 Hkv) d]``, ``out [N, T, H d]`` -> (``G`` in fp64, its elementwise bound)."""
    V, N, T, E = M.shape
    d, R = E // H, H // Hkv
    dd = dead(T, lengths, N)[:, :, None]
    q, k, v = gr.split(qkv.to(F64).masked_fill(dd, 0.0), H, Hkv)
    dO, O = gr.heads(M.to(F64).masked_fill(dd, 0.0), Hkv, R), gr.heads(out.to(F64).masked_fill(dd, 0.0), Hkv, R)
    a = abs(scale)
    mask = _hidden(N, T, lengths, causal, window)
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
    Pt, dSt = P.transpose(-1, -2), dS.transpose(-1, -2)
    dV = (Pt @ dO).sum(3)
    e_dV = (e_P.transpose(-1, -2) @ dO.abs()).sum(3) + (R * T + 2) * EPS * (Pt @ dO.abs()).sum(3)
    dK = (dSt @ q).sum(3) * scale
    e_dK = a * ((e_dS.transpose(-1, -2) @ q.abs()).sum(3) + (R * T + 3) * EPS * (dSt.abs() @ q.abs()).sum(3))
    G, bound = gr.pack(dQ, dK, dV), gr.pack(e_dQ, e_dK, e_dV) + FLT_MIN
    return G.masked_fill(dd, 0.0), bound.masked_fill(dd, FLT_MIN)


def make_case(seed, V, N, T, H, Hkv, d, scale=None, causal=False, lengths=None, window=None, qk_gain=1.0):
    """Seeded fp32 operands (CPU): ``(M, qkv, out, scale)``; the data of the dead positions is ordinary (finite) data, ``out`` is the
    masked forward pass (zero rows there)."""
    g = gen(seed)
    E = H * d
    qkv = torch.randn(N, T, (H + 2 * Hkv) * d, generator=g)
    qkv[..., :(H + Hkv) * d] *= qk_gain
    M = torch.randn(V, N, T, E, generator=g) * 10.0 ** (torch.rand(V, N, T, E, generator=g) * 2 - 1)
    scale = d ** -0.5 if scale is None else scale
    return M, qkv, forward(qkv, H, Hkv, scale, causal, lengths, window), scale


def case_operands(case):
    """``(M, qkv, out, scale, Hkv_eff)`` of a case of the list (``Hkv_eff = H`` for the multi-head call)."""
    T, d, H, Hkv, V, N, causal, scale, lengths, window = case
    He = H if Hkv is None else Hkv
    return make_case(1000 * T + d + H + (window or 0), V, N, T, H, He, d, scale, causal, lengths, window) + (He,)
