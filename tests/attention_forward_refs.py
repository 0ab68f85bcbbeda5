"""Derived error bounds for the fused attention forward pass (csrc/attention_forward.hip, ``vivit_attention_forward_f32`` and
``vivit_attention_cross_forward_f32``).  TEST INFRASTRUCTURE shared by tests/test_attention_forward_refs_host.py,
tests/test_attention_forward_gpu.py and tests/test_attention_forward_layers.py.  It holds only the bound: the cases, the masks, the
layouts and the fp64 forward passes are those of tests/attention_scoremod_refs.py and tests/attention_cross_refs.py.

The derivation of tests/attention_refs.py and tests/attention_scoremod_refs.py (eps = 2^-24, first order, elementwise against fp64)
carried one step further.  With ``e_s`` the error of a visible logit (``e_S`` of the plain function, ``e_s`` behind a cap and a table)
and ``e_lse``, ``e_P`` as those modules have them, unchanged:
* the kernel never forms ``P = exp(s - lse)``: it forms ``p_j = exp(s_j - m)`` with the running maximum ``m`` of the key blocks so far,
  multiplies what it has by ``alpha = exp(m_old - m_new)`` at each later key block and divides by ``l = sum_j p_j`` at the end.  The
  rounded arguments of these exponentials -- ``s_j - m`` and the ``m_old - m_new`` behind it, all >= 0 in magnitude and adding up to
  ``m_final - s_j <= lse - s_j`` -- change the term by at most ``eps |s_j - lse|`` relative, which is the term ``eps |S - lse|`` of
  ``e_P``; expf is the 2 eps of ``e_P``; the relative error of ``l`` is what ``e_lse`` bounds (``d lse = dl / l``).  So ``e_P`` bounds the
  error of the weight ``p_j / l`` the kernel applies, before the roundings of the accumulation, which ``gamma`` counts:
* ``out[i, c] = sum_j P_ij v_jc``: a dot product over the ``n_i`` visible keys of row i ((n_i + 2) eps, in any order and with or
  without fused multiply-adds: the convention of tests/attention_refs.py), at each of the at most ``KB = ceil(Tk / 32)`` visited key
  blocks one rescaling, which rounds ``alpha`` (expf: 2 eps) and the product (eps), and the final division (eps):
      gamma_i = (n_i + 2 + 3 KB + 1) eps,     e_out[i, c] = sum_j e_P[i, j] |v[j, c]| + gamma_i sum_j P[i, j] |v[j, c]| + 2^-126.
* ``lse = m + log l`` is computed as the rule's own first launch computes it: ``e_lse`` as it stands (+ 2^-126).
Rows of dead queries: reference 0, bound 2^-126 -- only an exact zero passes.  Every constant comes from counting roundings or from
the measured ``KAPPA`` of tests/attention_scoremod_refs.py; none comes from the outcome of a run.
"""
import math

import torch

import attention_cross_refs as cr
import attention_scoremod_refs as sr
from attention_scoremod_refs import BLOCK, EPS, F64, FLT_MIN, KAPPA, within   # noqa: F401  (within: re-exported for the test modules)


def _bounds(S, e_S, v, mask):
    """``S``, ``e_S [N, Hkv, R, Tq, Tk]`` (masked: -inf and 0), ``v [N, Hkv, 1, Tk, d]``, ``mask`` (broadcasts over S) ->
    ``(out [N, Tq, H d], e_out, lse [N, H, Tq], e_lse)`` in fp64."""
    N, Tq, Tk = S.shape[0], S.shape[-2], S.shape[-1]
    lse = torch.logsumexp(S, -1, keepdim=True)
    arg = (S - lse).masked_fill(mask, 0.0)
    P = torch.exp(S - lse)
    KB, lnT = math.ceil(Tk / BLOCK), math.log(max(Tk, 2))
    e_lse = e_S.amax(-1, keepdim=True) + EPS * (lse.abs() + Tk + 4 + KB * (lnT + 5) + 3 * lnT)
    e_P = (P * (e_S + e_lse + EPS * (arg.abs() + 2)) + FLT_MIN).masked_fill(mask, 0.0)
    n_vis = (~mask).expand_as(S).sum(-1, keepdim=True)
    gamma = EPS * (n_vis + 2 + 3 * KB + 1)
    rows = lambda t: t.movedim(-2, 1).reshape(N, Tq, -1)   # noqa: E731
    return rows(P @ v), rows(e_P @ v.abs() + gamma * (P @ v.abs())) + FLT_MIN, lse.reshape(N, -1, Tq), e_lse.reshape(N, -1, Tq) + FLT_MIN


def _kill(dq, out, e_out, lse, e_lse):
    """The rows of the dead queries ``dq [N, Tq]``: reference 0, bound 2^-126."""
    return (out.masked_fill(dq[:, :, None], 0.0), e_out.masked_fill(dq[:, :, None], FLT_MIN), lse.masked_fill(dq[:, None, :], 0.0),
            e_lse.masked_fill(dq[:, None, :], FLT_MIN))


def self_forward(qkv, H, Hkv, scale, causal, lengths=None, window=None, cap=None, table=None):
    """``qkv [N, T, (H + 2 Hkv) d]`` fp32 -> ``(out, e_out, lse, e_lse)`` of ``kernels.attention_forward``; the logits and their error
    are the lines of ``attention_scoremod_refs.rule``."""
    N, T, _ = qkv.shape
    d, R = qkv.shape[2] // (H + 2 * Hkv), H // Hkv
    dd = sr.dead(T, lengths, N)
    q, k, v = sr.gr.split(qkv.to(F64).masked_fill(dd[:, :, None], 0.0), H, Hkv)
    mask = sr.mr._hidden(N, T, lengths, causal, window)
    _, u, _, g, s = sr._scores(q, k, scale, cap, table, Hkv, R)
    e_z = (d + 3) * EPS * abs(scale) * (q.abs() @ k.abs().transpose(-1, -2))
    e_u = e_z if cap is None else g * e_z + KAPPA * EPS * u.abs()
    e_s = e_u if table is None else e_u + EPS * s.abs()
    return _kill(dd, *_bounds(s.masked_fill(mask, float("-inf")), e_s.masked_fill(mask, 0.0), v, mask))


def cross_forward(q, kv, H, Hkv, scale, query_lengths=None, key_lengths=None):
    """``q [N, Tq, H d]``, ``kv [N, Tk, 2 Hkv d]`` fp32 -> ``(out, e_out, lse, e_lse)`` of ``kernels.cross_attention_forward``; the
    logits and their error are the lines of ``attention_cross_refs.rule``."""
    N, Tq, Tk = q.shape[0], q.shape[1], kv.shape[1]
    d = q.shape[2] // H
    dq, dk = cr.dead(Tq, Tk, query_lengths, key_lengths, N)
    qh, k, v = cr.split(q.to(F64).masked_fill(dq[:, :, None], 0.0), kv.to(F64).masked_fill(dk[:, :, None], 0.0), H, Hkv)
    mask = cr._hidden(dq, dk)
    S = ((qh @ k.transpose(-1, -2)) * scale).masked_fill(mask, float("-inf"))
    e_S = ((d + 3) * EPS * abs(scale) * (qh.abs() @ k.abs().transpose(-1, -2))).masked_fill(mask, 0.0)
    return _kill(dq, *_bounds(S, e_S, v, mask))
