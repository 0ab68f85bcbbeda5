"""References for the Mamba-2 SSD layer (csrc/ssd.hip), fp64 torch on the CPU, one time step at a time; no tests in this file.

``scan`` is the recurrence and ``rules`` the adjoint formulas of include/vivit_hip.h.  With ``majorant=True`` both are evaluated with
every term replaced by its absolute value (``|M|, |x|, |B|, |C|, |D|`` and ``|A|`` where A multiplies a term of ``g_dt``, ``F_A`` and
``F_dt_bias``; Delta and the decays ``exp(Delta A)`` unchanged).  The bound of a result is

    ``|got - ref| <= c (T + S + P + heads per group + 160) 2^-24 majorant``,   ``c = 2 + max Delta |A|``  over the case's inputs.

Where this comes from -- the rounding chain of ONE term of a result in units of u = 2^-24 relative to the term's own majorant (the
kernels form no difference of large sums: every part of ``e_t`` is a sum of terms of the majorant).
* Decays.  Delta, A and the prefix sums l_t are fp64; every exponent is an fp64 difference ``l_t - l_s`` rounded once, which the
  exponential turns into a relative error ``|l_t - l_s| u`` of the decay it sits on.  A term that travels from step s to step t
  carries one such decay inside a chunk and one per chunk boundary it crosses, and the exponents of these add up to at most
  ``sum_{s < r <= t} Delta_r |A| <= T max Delta |A|``.  That is the ``max Delta |A| * T`` of the product ``c * T``.
* Each decay also has expf's 1 ulp (2 u), its product with what it scales (1 u) and the addition to the carried state (1 u): 4 u for
  each of at most ``T / 32 + 2`` decays of the state chain and the same for the adjoint chain, which ``e_t`` joins: ``<= T / 4 + 16``.
* Contractions.  A matrix product over K adds at most K u to a term (fp32 accumulation); the longest chain a term passes is
  ``C B^T`` (S), the masked product with the factor or the 0/1 triangle (Q = 64 at most, twice) and one product over P:
  ``S + P + 128``.  The sums over time of the three factors add ``T``, the head fold ``heads per group``.
* Single roundings: Delta, sigmoid and A to fp32, ``Delta x``, ``W o (M Xd^T)``, the row scalings, ``A e``, ``. sigmoid``: below 16.
Together ``max Delta |A| T + 2 T + S + P + heads per group + 160 <= c (T + S + P + heads per group + 160)``: derived, not fitted."""
import torch
import torch.nn.functional as F

F64, EPS = torch.float64, 2.0 ** -24


def _operands(x, A_log, dt_bias, H, P, S, G, softplus, majorant):
    N, T = x.shape[:2]
    x = x.to(F64)
    X, dt = x[..., :H * P].reshape(N, T, H, P), x[..., H * P:H * P + H] + dt_bias.to(F64)
    B, C = (x[..., H * P + H + i * G * S:H * P + H + (i + 1) * G * S].reshape(N, T, G, S).repeat_interleave(H // G, 2) for i in (0, 1))
    delta = F.softplus(dt, threshold=float("inf")) if softplus else dt
    if majorant:
        X, B, C = X.abs(), B.abs(), C.abs()
    A = -torch.exp(A_log.to(F64))
    return X, dt, B, C, delta, A, torch.exp(delta * A)   # X [N, T, H, P]; dt, delta, decay [N, T, H]; B, C [N, T, H, S]; A [H]


def states(X, B, delta, decay):
    """``Hs_{-1}, Hs_0, .., Hs_{T-1}``, each ``[N, H, P, S]``."""
    hs = [X.new_zeros(X.shape[0], X.shape[2], X.shape[3], B.shape[3])]
    for t in range(X.shape[1]):
        hs.append(decay[:, t, :, None, None] * hs[-1] + (delta[:, t, :, None] * X[:, t])[..., None] * B[:, t, :, None, :])
    return hs


def scan(x, A_log, D, dt_bias, H, P, S, G=1, softplus=True, majorant=False):
    X, _, B, C, delta, _, decay = _operands(x, A_log, dt_bias, H, P, S, G, softplus, majorant)
    hs = states(X, B, delta, decay)
    D = D.to(F64).abs() if majorant else D.to(F64)
    y = torch.stack([(hs[t + 1] * C[:, t, :, None, :]).sum(-1) for t in range(X.shape[1])], 1) + D[:, None] * X
    return y.flatten(2)


def rules(M, x, A_log, D, dt_bias, H, P, S, G=1, softplus=True, majorant=False):
    """``(g [V, N, T, H P + H + 2 G S], F_A [V, N, H], F_D [V, N, H], F_dt_bias [V, N, H])``."""
    X, dt, B, C, delta, A, decay = _operands(x, A_log, dt_bias, H, P, S, G, softplus, majorant)
    V, (N, T) = M.shape[0], x.shape[:2]
    M, D = M.to(F64).reshape(V, N, T, H, P), D.to(F64)
    if majorant:
        M, D = M.abs(), D.abs()
    Am = A.abs() if majorant else A
    hs = states(X, B, delta, decay)
    sig = torch.sigmoid(dt) if softplus else torch.ones_like(dt)
    lam, FA, FD, Fb, rows = None, 0.0, 0.0, 0.0, [None] * T
    for t in range(T - 1, -1, -1):
        lam = M[:, :, t, :, :, None] * C[:, t, :, None, :] + (decay[:, t + 1, :, None, None] * lam if lam is not None else 0.0)
        lB = (lam * B[:, t, :, None, :]).sum(-1)                                   # [V, N, H, P]
        e = (lam * (decay[:, t, :, None, None] * hs[t])).sum((-1, -2))             # [V, N, H]
        g_x = delta[:, t, :, None] * lB + D[:, None] * M[:, :, t]
        g_dt = (Am * e + (X[:, t] * lB).sum(-1)) * sig[:, t]
        g_B = (delta[:, t, :, None] * (lam * X[:, t, :, :, None]).sum(-2)).reshape(V, N, G, H // G, S).sum(3)
        g_C = (hs[t + 1] * M[:, :, t, :, :, None]).sum(-2).reshape(V, N, G, H // G, S).sum(3)
        rows[t] = torch.cat((g_x.flatten(2), g_dt, g_B.flatten(2), g_C.flatten(2)), -1)
        FA, FD, Fb = FA + e * delta[:, t], FD + (M[:, :, t] * X[:, t]).sum(-1), Fb + g_dt
    return torch.stack(rows, 2), FA * Am, FD, Fb


def constant(x, A_log, dt_bias, H, P, S, G=1, softplus=True):
    _, _, _, _, delta, A, _ = _operands(x, A_log, dt_bias, H, P, S, G, softplus, False)
    return 2.0 + float((delta * A).abs().max())


def bound(majorant, x, A_log, dt_bias, H, P, S, G=1, softplus=True):
    return constant(x, A_log, dt_bias, H, P, S, G, softplus) * (x.shape[1] + S + P + H // G + 160) * EPS * majorant
