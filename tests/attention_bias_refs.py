"""fp64 reference and derived error bound for the factor of a LEARNED relative-position bias table (csrc/attention.hip,
``vivit_attention_bias_factor_f32``; ``kernels.attention_bias_factor``).  TEST INFRASTRUCTURE shared by
tests/test_attention_bias_refs_host.py, tests/test_attention_bias_rule_gpu.py and tests/test_attention_bias_layers.py; it builds on
tests/attention_scoremod_refs.py (the score function, the mask, the cases, KAPPA) and edits nothing there.

The function.  With ``s_ij = u_ij + B[h, j - i + T - 1]`` of that module (the table is added behind the cap), the table's factor is
    Gd[v, n, h, r] = sum_{(i, j) visible, j - i = r} dS[v, n, h, i, j],    dS = P o (dP - D),
the sums of the diagonals of ``dS`` -- of ``dS``, not of ``dZ = dS o (1 - t^2)`` -- and an index ``[2 T - 1]`` sends the distances to
the ``R`` columns of the result: ``Gb[v, n, h, b] = sum_{r: index[r + T - 1] = b} Gd[v, n, h, r]`` (a plain table: the identity, or a
shift into a longer table; T5: many distances share a bucket).  An index value outside ``[0, R)`` belongs to no column.

Error bound.  ``dS`` and ``e_dS`` are derived exactly as ``attention_scoremod_refs.rule`` derives them (the same lines, in the same
order).  A diagonal is a sum of at most ``T`` terms, and a column one more sum over its ``count`` distances; every term meets at most
``count + T`` additions.  On the pattern of that module's ``e_dQ``:
    e_Gb = sum_col e_dS + (count + T + 3) eps sum_col |dS| + FLT_MIN.
"""
import math

import torch

import attention_scoremod_refs as sr
from attention_scoremod_refs import BLOCK, EPS, F64, FLT_MIN, KAPPA, chunk, dead, gen, gr, misaligned, mr, visible, within   # noqa: F401

BUCKETS, BUCKET_MAX_DISTANCE = 8, 16   # of the cases that go through relative_position_buckets


def ds(M, qkv, out, H, Hkv, scale, causal, lengths=None, window=None, cap=None, table=None):
    """``dS`` and its elementwise bound ``e_dS``, both ``[V, N, H, T, T]`` in fp64: the lines of ``attention_scoremod_refs.rule`` up to
    ``e_dS``, unchanged.  ``table [H, 2 T - 1]`` is the effective table."""
    V, N, T, E = M.shape
    d, R = E // H, H // Hkv
    dd = dead(T, lengths, N)[:, :, None]
    q, k, v = gr.split(qkv.to(F64).masked_fill(dd, 0.0), H, Hkv)
    dO, O = gr.heads(M.to(F64).masked_fill(dd, 0.0), Hkv, R), gr.heads(out.to(F64).masked_fill(dd, 0.0), Hkv, R)
    a = abs(scale)
    mask = mr._hidden(N, T, lengths, causal, window)
    z, u, t, g, s = sr._scores(q, k, scale, cap, table, Hkv, R)
    e_z = (d + 3) * EPS * a * (q.abs() @ k.abs().transpose(-1, -2))
    e_u = e_z if cap is None else g * e_z + KAPPA * EPS * u.abs()
    e_s = e_u if table is None else e_u + EPS * s.abs()
    S, e_S = s.masked_fill(mask, float("-inf")), e_s.masked_fill(mask, 0.0)
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
    # only visible pairs are summed (a dead query keeps its own position in the softmax: its dS is P (0 - 0))
    vis = visible(T, lengths, causal, window).expand(N, T, T)[None, :, None]
    return (dS.reshape(V, N, H, T, T).masked_fill(~vis, 0.0), e_dS.reshape(V, N, H, T, T).masked_fill(~vis, 0.0))


def diagonals(X):
    """``X [..., T, T]`` -> ``[..., 2 T - 1]``: entry ``r + T - 1`` is the sum of the entries with ``j - i = r``, diagonal by diagonal."""
    T = X.shape[-1]
    return torch.stack([torch.diagonal(X, offset=r, dim1=-2, dim2=-1).sum(-1) for r in range(-(T - 1), T)], -1)


def factor(M, qkv, out, H, Hkv, scale, causal, lengths, window, cap, table, index, R):
    """-> (``Gb [V, N, H, R]`` in fp64, its elementwise bound).  ``table [H, 2 T - 1]``: the effective table; ``index``: ``2 T - 1``
    integers, the column of each distance (a value outside ``[0, R)``: no column)."""
    T = M.shape[2]
    dS, e_dS = ds(M, qkv, out, H, Hkv, scale, causal, lengths, window, cap, table)
    Gd, e_Gd, a_Gd = diagonals(dS), diagonals(e_dS), diagonals(dS.abs())
    index = torch.as_tensor(index).long()
    assert tuple(index.shape) == (2 * T - 1,)
    Gb, bound = torch.zeros(*Gd.shape[:-1], R, dtype=F64), torch.zeros(*Gd.shape[:-1], R, dtype=F64)
    for b in range(R):
        sel = index == b
        count = int(sel.sum())
        if count:
            Gb[..., b] = Gd[..., sel].sum(-1)
            bound[..., b] = e_Gd[..., sel].sum(-1) + (count + T + 3) * EPS * a_Gd[..., sel].sum(-1)
    return Gb, bound + FLT_MIN


def visible_distances(T, lengths, causal, window):
    """``[N, 2 T - 1]`` bool (``[1, ...]`` without lengths): some visible pair of the sample has the distance ``j - i = r``."""
    return diagonals(visible(T, lengths, causal, window).to(F64)) > 0


def bucket_index(T, causal):
    """The index of the cases that go through buckets: T5's, eight buckets, bidirectional unless causal."""
    from vivit_amd.backend import relative_position_buckets
    return relative_position_buckets(T, BUCKETS, BUCKET_MAX_DISTANCE, not causal)


def _cases():
    """The cases of ``attention_scoremod_refs.CASES`` with ``bucketed`` appended: every third one reads a ``[H, 8]`` table through
    buckets; a case without a table gets the seeded "normal" one (the two ALiBi cases keep theirs)."""
    return [case[:11] + (case[11] or "normal", k % 3 == 2) for k, case in enumerate(sr.CASES)]


# Nothing is larger than T = 161, H = 6, d = 128, V = 9, N = 4 (the last case of the list: V = 5).
CASES = _cases()


def case_operands(case):
    """``(M, qkv, out, scale, Hkv_eff, param, table, index, R)`` of a case: ``param`` is the table as the module holds it
    (``[H, 2 T - 1]`` or ``[H, 8]``), ``table [H, 2 T - 1]`` the effective one, ``index`` (int64 ``[2 T - 1]``) the column of ``param``
    each distance reads, ``R = param.shape[1]``; ``out`` is the forward pass with the effective table."""
    T, d, H, Hkv, V, N, causal, scale, lengths, window, cap, kind, bucketed = case
    He = H if Hkv is None else Hkv
    seed = 1000 * T + d + H + (window or 0)
    if bucketed:
        param, index = torch.randn(H, BUCKETS, generator=gen(seed + 78)) * 3.0, bucket_index(T, causal)
        table = param[:, index].contiguous()
    else:
        param = table = sr.make_table(kind, seed, H, T)
        index = torch.arange(2 * T - 1)
    return sr.make_case(seed, V, N, T, H, He, d, scale, causal, lengths, window, cap, table) + (He, param, table, index, param.shape[1])
