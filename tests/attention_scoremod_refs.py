"""fp64 reference and derived error bounds for the attention rule with score modifiers -- a logit cap and a relative-position bias
table -- (csrc/attention.hip, ``vivit_attention_scoremod_jac_t_f32``) and for the activation kind ``"softcap"``.  TEST INFRASTRUCTURE
shared by tests/test_attention_scoremod_refs_host.py, tests/test_attention_scoremod_rule_gpu.py and
tests/test_attention_scoremod_layers.py; it builds on tests/attention_masked_refs.py (the mask, the dead positions, the helpers) and
tests/attention_gqa_refs.py (the layout), and edits neither.

The function.  Per sample and query head ``h`` of group ``g``, with ``z_ij = scale q_i k_j``:
    u = c tanh(z / c)  for a cap c > 0 (none: u = z),    s_ij = u_ij + B[h, j - i + T - 1]  for a table B [H, 2 T - 1] (none: s = u),
then the mask of tests/attention_masked_refs.py exactly as it is, and ``P = softmax_rows(s)``: the cap comes before the bias and both
before the mask.  The rule, with ``t = u / c``, ``g = 1 - t^2`` and the ``dO``, ``D``, ``dP`` of the plain rule:
    dS = P o (dP - D),   dZ = dS o g  (no cap: dZ = dS),   dQ_h = scale dZ K_g,   dK_g = scale sum_h dZ_h^T Q_h,   dV_g = sum_h P_h^T dO_h.
The table is a constant; it receives nothing.

Error bounds: the derivation of tests/attention_refs.py (carried to groups and masks by the two modules above), with ``e_z`` its
``e_S = (d + 3) eps |scale| (|Q| |K|^T)`` and these steps added:
* u = c tanh(z / c).  The error of z passes through the slope g of the map; the quotient, tanhf and the product round the result,
  which KAPPA counts in units of eps |u| (see KAPPA):                                      e_u = g e_z + KAPPA eps |u|.
* s = u + B, one addition of an exact table entry:                                         e_s = e_u + eps |s|.
  e_s takes the place of e_S in e_lse and e_P, unchanged otherwise.
* g = 1 - t^2 in ABSOLUTE terms (the factor cancels as |t| -> 1, a relative bound would be void there): t = u / c carries
  e_t = e_u / c, the square moves by 2 |t| e_t, and the product and the subtraction round numbers <= 1:   e_g = 2 |t| e_t + 2 eps.
* dZ = dS g, one more product:                                                             e_dZ = e_dS g + |dS| e_g + eps |dZ|,
  which takes the place of e_dS in e_dQ and e_dK.  (The kernels form P g first and multiply by dP - D; to first order the same
  three terms, with the roundings counted in e_dS's own 2 eps |dS|.)
Without a cap g = 1, e_g = 0 and e_u = e_z; without a table s = u and e_s = e_u: the bounds of tests/attention_masked_refs.py.
"""
import math

import torch

import attention_masked_refs as mr
from attention_masked_refs import BLOCK, D_MAX, EPS, F64, FLT_MIN, chunk, dead, gen, gr, misaligned, visible, within   # noqa: F401

# The error of the device's tanhf in units of eps = 2^-24 relative (half an ulp), for the bound e_u above.  The ROCm installation this
# was written on ships no accuracy statement for its device math library, so it was MEASURED once on an MI355X (ROCm 7.2): every
# float x with 2^-40 <= |x| <= 2^7, both signs (the arguments z / c of the cases lie within; beyond, tanhf is +-1), through tanhf on
# the device against tanh in fp64 on the device: the largest |tanhf(x) - tanh(x)| / (2^-24 |tanh(x)|) is 2.486, at x = 0.6352 -- an
# implementation good to 1.25 ulp.  DOUBLED: 4.972, written as 5.  The same scan of the whole expression c * tanhf(x / c) as the
# kernel writes it (a correctly rounded quotient before and a product behind, half an ulp each), for c in {0.5, 0.7, 1.5, 2, 3, 30,
# 50, 10^4}, gave at most 3.885 (c = 30), which the constant covers.  It comes from that scan alone, not from the outcome of a test.
KAPPA = 5.0

CAPS = (1.5, 0.7, 50.0, 3.0)   # 50 is Gemma-2's (nearly inert on unit data); the others bend unit-scale logits
T_ALL = mr.T_ALL
HEADS = mr.HEADS
DIMS = mr.DIMS


def _cases():
    """(T, d, H, Hkv, V, N, causal, scale, lengths, window, cap, table); ``table``: None, "normal" (random normals times 3, so that
    both ends j - i = +-(T - 1) carry weight) or "alibi"."""
    spec = [(1, None, False, (1, 0), "cb"), (1, None, True, None, "c"), (5, 2, True, (5, 1, 0), "b"), (5, None, False, (5, 5), "cb"),
            (32, 2, False, (32, 31, 1), "c"), (32, None, True, (32, 0, 31), "a"), (33, 33, True, (33, 32, 31, 1), "cb"),
            (33, 2, False, (0, 33, 32), "b"), (33, None, True, None, "c"), (65, 33, True, (65, 64, 33, 0), "c"),
            (65, 65, False, (65, 65), "b"), (65, 2, True, None, "cb"), (65, None, False, (64, 65, 32), "cb"),
            (97, 33, False, (97, 65, 33, 0), "cb"), (97, 65, True, (97, 64), "b"), (97, None, True, (1, 97, 32), "c"),
            (97, 2, False, None, "b"), (161, 65, False, (161, 64, 31, 1), "cb"), (161, 33, True, (65, 161, 33), "b"),
            (161, None, True, (32, 64, 65, 161), "b"), (161, None, False, (161, 65, 0, 161), "cb"), (161, 2, True, None, "c"),
            (161, 65, True, (161, 0, 97), "c"), (97, 33, True, None, "ca")]
    cases = []
    for k, (T, W, causal, lengths, mod) in enumerate(spec):
        d, (H, Hkv) = DIMS[k % 8], HEADS[k % 5]
        c = chunk(d)
        V = c - 1 if (k // 8 + k) % 2 == 0 else 2 * c + 1
        N = 2 if lengths is None else len(lengths)
        cap = CAPS[k % 4] if "c" in mod else None
        table = "normal" if "b" in mod else "alibi" if "a" in mod else None
        cases.append((T, d, H, Hkv, V, N, causal, -0.5 if k == 7 else None, lengths, W, cap, table))
    # the largest shape of the list: both modifiers, a window, mixed lengths
    cases.append((161, 128, 6, 3, 5, 4, True, None, (161, 64, 31, 1), 33, 1.5, "normal"))
    return cases


# The cases of tests/test_attention_scoremod_rule_gpu.py (shared with the host test, which checks this rule), by the rule of
# attention_masked_refs.CASES: T in {1, 5, 32, 33, 65, 97, 161}; every instance of the kernel meets its smallest and its largest d;
# the multi-head call and grouped queries with R in {1, 2, 4}; a V of one chunk minus one and of two chunks plus one; a cap alone, a
# table alone and both, each with the causal mask, with the windows 2, 33 and 65 and with mixed lengths that include 0 and T; one
# negative scale; random tables and two ALiBi tables.  Nothing is larger than T = 161, H = 6, d = 128, V = 9, N = 4.
CASES = _cases()


def bias_matrix(table, T):
    """``table [H, 2 T - 1]`` -> ``[H, T, T]`` with ``[h, i, j] = table[h, j - i + T - 1]``, entry by entry from the definition."""
    H = table.shape[0]
    assert tuple(table.shape) == (H, 2 * T - 1)
    B = torch.empty(H, T, T, dtype=table.dtype)
    for i in range(T):
        B[:, i, :] = table[:, T - 1 - i:2 * T - 1 - i]
    return B


def make_table(kind, seed, H, T):
    """The fp32 table of a case (CPU), ``None`` for none."""
    if kind is None:
        return None
    if kind == "alibi":
        from vivit_amd.backend import alibi_bias
        return alibi_bias(H, T)
    return torch.randn(H, 2 * T - 1, generator=gen(seed + 77)) * 3.0


def _scores(q, k, scale, cap, table, Hkv, R):
    """z, u, t, g, s (all fp64, unmasked, ``[N, Hkv, R, T, T]``) from the split operands."""
    T = q.shape[-2]
    z = (q @ k.transpose(-1, -2)) * scale
    if cap is None:
        u, t, g = z, torch.zeros_like(z), torch.ones_like(z)
    else:
        t = torch.tanh(z / cap)
        u, g = cap * t, 1.0 - t * t
    s = u if table is None else u + bias_matrix(table.to(F64), T).view(Hkv, R, T, T)
    return z, u, t, g, s


def forward(qkv, H, Hkv, scale, causal, lengths=None, window=None, cap=None, table=None):
    """The module output in the dtype of ``qkv`` (``[N, T, (H + 2 Hkv) d] -> [N, T, H d]``), rows of zeros at the dead positions."""
    N, T, _ = qkv.shape
    dd = dead(T, lengths, N)
    q, k, v = gr.split(qkv.masked_fill(dd[:, :, None], 0.0), H, Hkv)
    s = _scores(q, k, scale, cap, None if table is None else table.to(qkv.dtype), Hkv, H // Hkv)[4].to(qkv.dtype)
    s = s.masked_fill(mr._hidden(N, T, lengths, causal, window), float("-inf"))
    return (s.softmax(-1) @ v).movedim(-2, 1).reshape(N, T, -1).masked_fill(dd[:, :, None], 0.0)


def rule(M, qkv, out, H, Hkv, scale, causal, lengths=None, window=None, cap=None, table=None):
    """``M [V, N, T, H d]``, ``qkv [N, T, (H + 2 Hkv) d]``, ``out [N, T, H d]`` -> (``G`` in fp64, its elementwise bound)."""
    V, N, T, E = M.shape
    d, R = E // H, H // Hkv
    dd = dead(T, lengths, N)[:, :, None]
    q, k, v = gr.split(qkv.to(F64).masked_fill(dd, 0.0), H, Hkv)
    dO, O = gr.heads(M.to(F64).masked_fill(dd, 0.0), Hkv, R), gr.heads(out.to(F64).masked_fill(dd, 0.0), Hkv, R)
    a = abs(scale)
    mask = mr._hidden(N, T, lengths, causal, window)
    z, u, t, g, s = _scores(q, k, scale, cap, table, Hkv, R)
    e_z = (d + 3) * EPS * a * (q.abs() @ k.abs().transpose(-1, -2))
    if cap is None:
        e_u, e_g = e_z, torch.zeros_like(z)
    else:
        e_u = g * e_z + KAPPA * EPS * u.abs()
        e_g = 2 * t.abs() * (e_u / cap) + 2 * EPS
    e_s = e_u if table is None else e_u + EPS * s.abs()
    S, e_S = s.masked_fill(mask, float("-inf")), e_s.masked_fill(mask, 0.0)
    # from here on tests/attention_masked_refs.py, with dZ in the place of dS in dQ and dK
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
    dZ, e_dZ = dS, e_dS
    if cap is not None:
        dZ = dS * g
        e_dZ = e_dS * g + dS.abs() * e_g + EPS * dZ.abs()
    dQ = (dZ @ k) * scale
    e_dQ = a * (e_dZ @ k.abs() + (T + 3) * EPS * (dZ.abs() @ k.abs()))
    Pt, dZt = P.transpose(-1, -2), dZ.transpose(-1, -2)
    dV = (Pt @ dO).sum(3)
    e_dV = (e_P.transpose(-1, -2) @ dO.abs()).sum(3) + (R * T + 2) * EPS * (Pt @ dO.abs()).sum(3)
    dK = (dZt @ q).sum(3) * scale
    e_dK = a * ((e_dZ.transpose(-1, -2) @ q.abs()).sum(3) + (R * T + 3) * EPS * (dZt.abs() @ q.abs()).sum(3))
    G, bound = gr.pack(dQ, dK, dV), gr.pack(e_dQ, e_dK, e_dV) + FLT_MIN
    return G.masked_fill(dd, 0.0), bound.masked_fill(dd, FLT_MIN)


def mean_t2(qkv, H, Hkv, scale, cap):
    """The mean of t^2 = tanh^2(z / c) over all pairs: how much of the cap's derivative a case feels."""
    q, k, _ = gr.split(qkv.to(F64), H, Hkv)
    return float((torch.tanh((q @ k.transpose(-1, -2)) * scale / cap) ** 2).mean())


def make_case(seed, V, N, T, H, Hkv, d, scale=None, causal=False, lengths=None, window=None, cap=None, table=None, qk_gain=1.0):
    """Seeded fp32 operands (CPU): ``(M, qkv, out, scale)``, the operands of attention_masked_refs.make_case for the same seed with
    ``out`` the modified forward pass."""
    M, qkv, _, scale = mr.make_case(seed, V, N, T, H, Hkv, d, scale, causal, lengths, window, qk_gain)
    return M, qkv, forward(qkv, H, Hkv, scale, causal, lengths, window, cap, table), scale


def case_operands(case):
    """``(M, qkv, out, scale, Hkv_eff, table)`` of a case of the list (``Hkv_eff = H`` for the multi-head call)."""
    T, d, H, Hkv, V, N, causal, scale, lengths, window, cap, kind = case
    He = H if Hkv is None else Hkv
    seed = 1000 * T + d + H + (window or 0)
    table = make_table(kind, seed, H, T)
    return make_case(seed, V, N, T, H, He, d, scale, causal, lengths, window, cap, table) + (He, table)


# ---- the activation kind "softcap": out = M (1 - tanh^2(x / cap)) --------------------------------------------------------------------
def act_softcap(M, x, cap):
    """``M [V, *x.shape]``, ``x`` -> (``out`` in fp64, its elementwise bound).  t = tanhf(x / cap) carries (KAPPA + 1) eps |t| (the
    rounded quotient moves tanh by at most eps |t|, since y (1 - tanh^2 y) <= tanh y), g = 1 - t^2 therefore 2 |t| e_t + 2 eps in
    absolute terms, and the product with M rounds once."""
    t = torch.tanh(x.to(F64) / cap)
    g = 1.0 - t * t
    e_g = 2 * t.abs() * ((KAPPA + 1) * EPS * t.abs()) + 2 * EPS
    m = M.to(F64)
    return m * g, m.abs() * (e_g + EPS * g) + FLT_MIN
