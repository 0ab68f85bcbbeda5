"""References for the selective scan (csrc/selective_scan.hip), fp64 torch on the CPU; no tests in this file.

``scan`` is the plain loop, ``rules`` the adjoint formulas of include/vivit_hip.h, and with ``majorant=True`` both are evaluated with
every term replaced by its absolute value (``|M|, |u|, |B|, |C|, |Dk|`` and ``|A|`` where A multiplies a term of ``g_dt`` and ``F_A``;
the decays ``exp(Delta A)`` unchanged).  The bound of a result is

    ``|got - ref| <= c (T + S + 4) 2^-24 majorant``,   ``c = 6 + max Delta |A|``  over the case's inputs.

Where c comes from -- the rounding of ONE time step of a term, in units of 2^-24 relative to the term's majorant.  The kernels
evaluate Delta (softplus), A = -exp(A_log) and sigmoid(dt) in fp64 and round the fp64 product Delta A once: the decay's argument
is off by ``|Delta A| 2^-24``, which the exponential turns into a relative error of ``max Delta |A|``; expf is documented at 1 ulp = 2
units.  The product ``decay * h`` (or ``decay * a``) is rounded (1) and the fmaf that adds the step's input (1): ``4 + max Delta |A|`` per
step for a propagated term; an input term has Delta to fp32 (1), ``Delta u`` (1) and the fmaf (1), which is less.  A term of a rule
passes at most T steps (t steps of h and T - t of a, joined by ``e = a p``), so ``(4 + max Delta |A|) T`` covers the chains.  What is
left are sums: at most S terms over the states and T over time (one rounding each, hence one more unit of c against ``T + S``), the
tree over the 64 channels of a block (6 levels), the channel blocks, and the single products ``e Delta``, ``. A``, ``. sigmoid``,
``Dk M`` with the rounding of A, sigmoid and Delta to fp32: below ``2 (S + 4)`` for up to 4 blocks, the second unit.  Hence c = 6 +
max Delta |A|, below the 8 + 2 max Delta |A| the layer's specification allows, and not fitted to any outcome."""
import torch
import torch.nn.functional as F

F64, EPS = torch.float64, 2.0 ** -24


def split(x, D, S):
    return x[..., :D], x[..., D:2 * D], x[..., 2 * D:2 * D + S], x[..., 2 * D + S:]


def _operands(x, A_log, softplus, majorant):
    D, S = A_log.shape
    u, dt, B, C = split(x.to(F64), D, S)
    delta = F.softplus(dt, threshold=float("inf")) if softplus else dt
    A = -torch.exp(A_log.to(F64))
    if majorant:
        u, B, C = u.abs(), B.abs(), C.abs()
    return u, dt, B, C, delta, A, torch.exp(delta[..., None] * A)   # decay [N, T, D, S]


def states(u, B, delta, decay):
    """``h_{-1}, h_0, .., h_{T-1}``, each ``[N, D, S]``."""
    hs = [torch.zeros_like(decay[:, 0])]
    for t in range(u.shape[1]):
        hs.append(decay[:, t] * hs[-1] + (delta[:, t] * u[:, t])[..., None] * B[:, t, None, :])
    return hs


def scan(x, A_log, Dk, softplus=True, majorant=False):
    u, _, B, C, delta, _, decay = _operands(x, A_log, softplus, majorant)
    hs = states(u, B, delta, decay)
    Dk = Dk.to(F64).abs() if majorant else Dk.to(F64)
    return torch.stack([(hs[t + 1] * C[:, t, None, :]).sum(-1) for t in range(u.shape[1])], 1) + Dk * u


def rules(M, x, A_log, Dk, softplus=True, majorant=False):
    """``(g [V, N, T, 2 D + 2 S], F_A [V, N, D, S], F_Dk [V, N, D])``."""
    u, dt, B, C, delta, A, decay = _operands(x, A_log, softplus, majorant)
    M, Dk = M.to(F64), Dk.to(F64)
    if majorant:
        M, Dk = M.abs(), Dk.abs()
    Am = A.abs() if majorant else A
    hs, T = states(u, B, delta, decay), u.shape[1]
    sig = torch.sigmoid(dt) if softplus else torch.ones_like(dt)
    a, FA, rows = None, 0.0, [None] * T
    for t in range(T - 1, -1, -1):
        a = M[:, :, t, :, None] * C[:, t, None, :] + (decay[:, t + 1] * a if a is not None else 0.0)   # [V, N, D, S]
        e = a * decay[:, t] * hs[t]
        aB = (a * B[:, t, None, :]).sum(-1)
        g_u = aB * delta[:, t] + Dk * M[:, :, t]
        g_dt = ((e * Am).sum(-1) + u[:, t] * aB) * sig[:, t]
        g_B = (a * (delta[:, t] * u[:, t])[..., None]).sum(2)
        g_C = (M[:, :, t, :, None] * hs[t + 1]).sum(2)
        rows[t] = torch.cat((g_u, g_dt, g_B, g_C), -1)
        FA = FA + e * delta[:, t, :, None]
    return torch.stack(rows, 2), FA * Am, (M * u).sum(2)


def constant(x, A_log, softplus=True):
    _, _, _, _, delta, A, _ = _operands(x, A_log, softplus, False)
    return 6.0 + float((delta[..., None] * A).abs().max())


def bound(majorant, x, A_log, softplus=True):
    T, S = x.shape[1], A_log.shape[1]
    return constant(x, A_log, softplus) * (T + S + 4) * EPS * majorant
