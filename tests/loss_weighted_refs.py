"""fp64 references for the cross-entropy factors with ``ignore_index``, class ``weight``, ``label_smoothing`` and probability targets
(``vivit_ce_target_scales_f32`` and the ``_w`` entry points of include/vivit_hip.h; ``_ce_position_weights`` of
vivit_amd/backend/extensions.py).  TEST INFRASTRUCTURE shared by tests/test_loss_weighted_refs_host.py (no GPU),
tests/test_loss_weighted_kernels_gpu.py and tests/test_loss_weighted_layers.py; in the manner of tests/loss_positions_refs.py, on
whose unweighted factors (``scale = 1``) everything here is built.

The Hessian of ``F.cross_entropy`` w.r.t. the logits of position ``i = (n, l)`` is ``omega_i (diag p_i - p_i p_i^T)``
(tests/test_loss_weighted_refs_host.py holds that to ``torch.autograd.functional.hessian``), so both factors are the unweighted ones
times ``sqrt(omega_i)`` at position ``i``; positions with ``omega_i = 0`` are zero BY ASSIGNMENT, never by a product (their logits may be
NaN).  With ``w`` the class weights (ones if absent), ``wbar = mean_c w_c``, ``eps`` the label smoothing:

* class-index targets ``y [N, *D]``: ``i`` counts iff ``y_i != ignore_index`` and ``0 <= y_i < C``; ``a_i = (1 - eps) w[y_i] + eps wbar``
  if it counts (exactly 1 without weights), else 0; ``norm = sum over counted i of w[y_i]`` ('mean', whole batch) or 1 ('sum');
  ``omega_i = a_i / norm``, and 0 where ``a_i = 0`` even if ``norm = 0``;
* probability targets ``t [N, C, *D]``: ``omega_i = sum_c w_c ((1 - eps) t_ic + eps / C) / norm``, ``norm = N L`` ('mean') or 1.
"""
import torch

import loss_positions_refs as base

F64 = torch.float64


def counted_positions(target, C, ignore_index):
    return (target != ignore_index) & (target >= 0) & (target < C)


def position_weights(target, C, weight=None, ignore_index=-100, eps=0.0, reduction="mean"):
    """omega (fp64, [N, *D]) for class-index (integer ``target [N, *D]``) or probability (floating ``target [N, C, *D]``) targets."""
    w = torch.ones(C, dtype=F64) if weight is None else weight.detach().cpu().to(F64)
    target = target.detach().cpu()
    if target.is_floating_point():
        t = target.to(F64).movedim(1, -1)                                       # [N, *D, C]
        a = (((1.0 - eps) * t + eps / C) * w).sum(-1)
        return a / (a.numel() if reduction == "mean" else 1)
    ok = counted_positions(target, C, ignore_index)
    omega = torch.zeros(target.shape, dtype=F64)
    wy = w[target[ok]]                                                          # (only counted targets index anything)
    a = torch.ones_like(wy) if weight is None else (1.0 - eps) * wy + eps * w.mean()
    norm = wy.sum() if reduction == "mean" else torch.ones((), dtype=F64)
    vals = a / norm
    vals[a == 0] = 0.0
    omega[ok] = vals
    return omega


def scale_factor(S, omega, mult=1):
    """The unweighted fp64 factor ``S [V, N, C, *D]`` (``scale = 1``) times ``sqrt(omega / mult)`` at every position; positions with
    ``omega == 0`` are assigned zero."""
    s = torch.sqrt(omega / mult).unsqueeze(0).unsqueeze(2)                      # [1, N, 1, *D]
    out = S * s
    dead = (omega == 0).unsqueeze(0).unsqueeze(2).expand_as(out)
    out[dead] = 0.0
    return out


def ce_exact_w(out, omega):
    """out [N, C, *D] (or [N, C]), omega [N, *D] -> fp64 S [C L, N, C, *D]."""
    flat = out.dim() == 2
    z = out.unsqueeze(-1) if flat else out
    S = scale_factor(base.ce_exact_vec(z, 1.0), omega.unsqueeze(-1) if flat else omega)
    return S.squeeze(-1) if flat else S


def ce_sampled_w(out, idx, omega):
    """out [N, C, *D] (or [N, C]), idx [M, N, *D], omega [N, *D] -> fp64 S [M, N, C, *D] with sqrt(omega / M)."""
    flat = out.dim() == 2
    z, k, om = (out.unsqueeze(-1), idx.unsqueeze(-1), omega.unsqueeze(-1)) if flat else (out, idx, omega)
    S = scale_factor(base.ce_sampled_vec(z, k.cpu(), 1.0), om, mult=idx.shape[0])
    return S.squeeze(-1) if flat else S


def target_scales(target, C, weight=None, ignore_index=-100, eps=0.0, mean=True, mult=1):
    """fp64 sqrt(omega / mult): what ``vivit_ce_target_scales_f32`` rounds to fp32."""
    return torch.sqrt(position_weights(target, C, weight, ignore_index, eps, "mean" if mean else "sum") / mult)


def loss_omega(lossf, target, C):
    """omega of an ``nn.CrossEntropyLoss`` instance."""
    return position_weights(target, C, lossf.weight, lossf.ignore_index, lossf.label_smoothing, lossf.reduction)


def exact_factor(out, lossf, target):
    return ce_exact_w(out, loss_omega(lossf, target, out.shape[1]))


def sampled_factor(out, idx, lossf, target):
    return ce_sampled_w(out, idx, loss_omega(lossf, target, out.shape[1]))


GUARD, GUARD_WORDS, guarded, guards_intact = base.GUARD, base.GUARD_WORDS, base.guarded, base.guards_intact
