"""fp64 references for the per-position loss-Hessian square roots (csrc/loss_positions.hip, ``_loss_hessian_sqrt_positions`` of
vivit_amd/backend/extensions.py).  TEST INFRASTRUCTURE shared by tests/test_loss_positions_refs_host.py (no GPU),
tests/test_loss_positions_kernels_gpu.py and tests/test_loss_positions_layers.py; in the manner of tests/llama_refs.py.

Every reference restates the formula of include/vivit_hip.h in torch fp64 with a plain loop over the positions (``ce_sampled_vec`` and
``ce_exact_vec`` are the same formulas without the loop, for the tests with 10^5 to 10^7 positions;
tests/test_loss_positions_refs_host.py holds them to the loops bit for bit): for an output
``[N, C, *D]`` with ``L = prod(D)`` positions and ``p[n, :, l] = softmax_c(out[n, :, l])``,

* cross entropy, exact (``V = C L``, row ``v = c' L + l'``):  ``S[v, n, c, l] = [l = l'] sqrt(p[n, c', l]) ([c = c'] - p[n, c, l]) scale``
* cross entropy, sampled (``V = M``, class indices ``idx [M, N, *D]``):  ``S[m, n, c, l] = (p[n, c, l] - [c = idx[m, n, l]]) scale``; an
  index outside ``[0, C)`` matches no class
* squared error, exact (``V = C L``):  ``S[v, n, :] = scale e_v``;  sampled:  ``S = scale eps``.

``scale`` is ``1 / sqrt(norm)`` (``1 / sqrt(M norm)`` sampled) with ``norm = N L`` for the mean cross entropy, and ``sqrt(2 / norm)``
(``sqrt(2 / (M norm))``) with ``norm = N C L`` for the mean squared error; ``norm = 1`` for ``reduction='sum'`` (:func:`norm_of`).
"""
import math

import torch

F64 = torch.float64


def norm_of(loss, reduction, N, C, L):
    if reduction == "sum":
        return 1
    return N * L if loss == "ce" else N * C * L


def ce_exact(out, scale):
    """out [N, C, *D] -> fp64 S [C L, N, C, *D]."""
    N, C, D = out.shape[0], out.shape[1], tuple(out.shape[2:])
    L = math.prod(D)
    z = out.to(F64).reshape(N, C, L)
    S = torch.zeros(C * L, N, C, L, dtype=F64)
    for n in range(N):
        for l in range(L):
            p = torch.softmax(z[n, :, l], 0)
            for cp in range(C):
                e = torch.zeros(C, dtype=F64)
                e[cp] = 1.0
                S[cp * L + l, n, :, l] = torch.sqrt(p[cp]) * (e - p) * scale
    return S.reshape(C * L, N, C, *D)


def ce_sampled(out, idx, scale):
    """out [N, C, *D], idx [M, N, *D] (any integer dtype) -> fp64 S [M, N, C, *D]."""
    N, C, D = out.shape[0], out.shape[1], tuple(out.shape[2:])
    L = math.prod(D)
    M = idx.shape[0]
    z = out.to(F64).reshape(N, C, L)
    k = idx.reshape(M, N, L)
    S = torch.zeros(M, N, C, L, dtype=F64)
    for n in range(N):
        for l in range(L):
            p = torch.softmax(z[n, :, l], 0)
            for m in range(M):
                e = torch.zeros(C, dtype=F64)
                if 0 <= int(k[m, n, l]) < C:
                    e[int(k[m, n, l])] = 1.0
                S[m, n, :, l] = (p - e) * scale
    return S.reshape(M, N, C, *D)


def _softmax_over_classes(z):
    """fp64 z [N, C, L] -> softmax over C.  Taken along the last axis of a contiguous [N, L, C], the arrangement in which torch sums
    the classes of a position in the order it uses for the single vector ``z[n, :, l]`` of the loops: the same bits."""
    return torch.softmax(z.movedim(1, 2).contiguous(), 2).movedim(2, 1)


def ce_sampled_vec(out, idx, scale):
    """:func:`ce_sampled` without the loop over the positions (for 10^5 to 10^7 of them): one fp64 ``torch.softmax`` over the classes
    and a comparison of the class numbers with the indices.  Non-finite logits follow torch: a NaN, a ``+inf`` or nothing but ``-inf``
    among the classes of a position makes every class of that position NaN; a ``-inf`` beside finite classes is a probability of 0."""
    N, C, D = out.shape[0], out.shape[1], tuple(out.shape[2:])
    L = math.prod(D)
    M = idx.shape[0]
    p = _softmax_over_classes(out.to(F64).reshape(N, C, L))
    hit = idx.reshape(M, N, 1, L) == torch.arange(C).view(1, 1, C, 1)          # (an index outside [0, C) equals no class number)
    return ((p.unsqueeze(0) - hit.to(F64)) * scale).reshape(M, N, C, *D)


def ce_exact_vec(out, scale):
    """:func:`ce_exact` without the loop over the positions.  The rows ``v = c' L + l'`` are written at ``l = l'`` only, so a NaN at one
    position leaves the structural zeros of every other position exactly 0.0 (a product with a mask would not)."""
    N, C, D = out.shape[0], out.shape[1], tuple(out.shape[2:])
    L = math.prod(D)
    p = _softmax_over_classes(out.to(F64).reshape(N, C, L))
    e = torch.eye(C, dtype=F64).view(C, 1, C, 1)                               # [c', 1, c, 1]
    block = torch.sqrt(p).movedim(1, 0).unsqueeze(2) * (e - p.unsqueeze(0)) * scale   # [c', n, c, l]
    S = torch.zeros(C, L, N, C, L, dtype=F64)
    pos = torch.arange(L)
    S[:, pos, :, :, pos] = block.movedim(3, 0)                                 # (the indexed axes lead: [l, c', n, c])
    return S.reshape(C * L, N, C, *D)


def mse_exact(shape, scale):
    """shape (N, C, *D) -> fp64 S [C L, N, C, *D] = scale I for every sample."""
    N, CL = shape[0], math.prod(shape[1:])
    return (scale * torch.eye(CL, dtype=F64)).unsqueeze(1).repeat(1, N, 1).reshape(CL, *shape)


def mse_sampled(eps, scale):
    return eps.to(F64) * scale


def exact_factor(out, loss, reduction="mean"):
    """The exact factor of ``loss`` in {"ce", "mse"} on out [N, C, *D], normalisation included."""
    N, C, L = out.shape[0], out.shape[1], math.prod(out.shape[2:])
    norm = norm_of(loss, reduction, N, C, L)
    if loss == "ce":
        return ce_exact(out, 1.0 / math.sqrt(norm))
    return mse_exact(tuple(out.shape), math.sqrt(2.0 / norm))


# ---- guarded outputs (as tests/llama_refs.py) -------------------------------------------------------------------------------------------
GUARD, GUARD_WORDS = -24601.0, 64    # (64 floats: the view keeps the 16-byte alignment of the buffer)


def guarded(numel, device, shift=False):
    """(buffer, flat view of ``numel`` floats pre-filled with NaN between guard words); ``shift``: the view 4 bytes off 16-byte
    alignment."""
    off = GUARD_WORDS + (1 if shift else 0)
    buf = torch.full((numel + 2 * GUARD_WORDS + 1,), GUARD, dtype=torch.float32, device=device)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + numel]
    view.fill_(float("nan"))
    return buf, view


def guards_intact(buf, view, shift=False):
    off = GUARD_WORDS + (1 if shift else 0)
    return bool((buf[:off] == GUARD).all()) and bool((buf[off + view.numel():] == GUARD).all())
