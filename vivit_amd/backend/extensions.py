"""Extensions of the stand-in backend: BatchGrad, SqrtGGN{Exact,MC}, ViViTGGN{Exact,MC}.

Data contract (identical to BackPACK's):
  ``param.grad_batch``       [N_grad, *param.shape]      carries 1/N for ``reduction='mean'``
  ``param.sqrt_ggn_exact``   [C, N_ggn, *param.shape]    carries 1/sqrt(N)
  ``param.sqrt_ggn_mc``      [M, N_ggn, *param.shape]    carries 1/sqrt(M N)
  ``param.vivit_ggn_exact|mc``  dict with closures ``gram_mat() -> [C,N,C,N]``,
      ``V_mat_prod(mat[F,C,N]) -> [F,*param]``, ``V_t_mat_prod(mat[F,*param]) -> [F,C,N]``
      (vivit/extensions/secondorder/vivit/base.py:126-130); Linear weights keep the factorised
      form ``s=[C,N,out], z=[N,in]`` (vivit/extensions/secondorder/vivit/linear.py:41-81); on sequence inputs
      ``[N,*,in]`` with a large explicit factor, ``s=[C,N,*,out], z=[N,*,in]`` (``_linear_seq_weight_closures``).
"""
import math
from typing import List, Optional, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from vivit_amd import _lib, kernels
from vivit_amd.backend.custom_module import (ActiveIdentity, Pad, Permute, ProductModule, RotaryEmbedding, ScaledDotProductAttention,
                                              ScaledDotProductCrossAttention, ScaleModule,
                                              Slicing, SoftCap, SumModule, _gqa_split)
from vivit_amd.utils.ggn import Vmp
from vivit_amd.utils.gram import mVp, pairwise_dot

DP_ROWS_MAX_COLUMNS = 4096  # data parallel: narrower materialised factors are all-gathered (block rows), wider ones
                            # go through the all-to-all to parameter shards (vivit_amd.distributed.BatchShardedGram)
# A Linear weight on a sequence input [N, T, in] (ViViTGGN*): an explicit factor [C, N, O, I] above SEQ_LINEAR_EXPLICIT_MAX_BYTES is
# never built (_linear_seq_weight_closures), and the Gram build's own scratch (a row slab of Gs on route A, a chunk of the factor on
# route B) stays within SEQ_LINEAR_WORKSPACE_BYTES.  Both are policies, not measurements; both are read at call time.
SEQ_LINEAR_EXPLICIT_MAX_BYTES = 64 << 20
SEQ_LINEAR_WORKSPACE_BYTES = 256 << 20
# Route A (expanded) is taken when SEQ_LINEAR_KAPPA * macs_A <= macs_B (_seq_linear_plan).  Measured
# (profiles/seq_linear_gram_time.log; N = 64, C = 10, (O, I) = (3072, 768) and (768, 3072), T in {4, 16, 64, 197}): route A is the
# faster of the two at the six shapes with macs_B / macs_A >= 0.224 and the slower at the two with macs_B / macs_A <= 0.123 (T = 197),
# so the planner never picks the slower one for kappa in (0.123, 0.224]; this is the smallest such value to three digits.  (A
# multiply-add of route A is the cheaper one: its products are large GEMMs, route B's are ninety small SYRKs and convolution rules.)
SEQ_LINEAR_KAPPA = 0.124
GEMM_PIECE_MIN_ROWS = 256   # _gemm_nt_within cuts a product no finer than this (read at call time)
_LOSSES = (nn.CrossEntropyLoss, nn.MSELoss)
_BATCHNORM = (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d)
_NORMS = (nn.LayerNorm, nn.GroupNorm)   # normalisations over each sample's own elements: no train / eval distinction
_CONVS = (nn.Conv1d, nn.Conv2d, nn.Conv3d, nn.ConvTranspose1d, nn.ConvTranspose2d, nn.ConvTranspose3d)


def subsample(tensor: Tensor, dim: int = 0, subsampling: Optional[List[int]] = None) -> Tensor:
    """``backpack.utils.subsampling.subsample`` (used at linear.py:42)."""
    if subsampling is None:
        return tensor
    idx = torch.as_tensor(subsampling, device=tensor.device, dtype=torch.long)
    return tensor.index_select(dim, idx)


class LinearFactor:
    """Factorised quantity of a Linear weight, ``T[..., n, o, i] = s[..., n, o] * z[n, i]``, never materialised.

    ``s: [C, N, out]`` for a sqrt-GGN factor (``V_t`` of vivit/extensions/secondorder/vivit/linear.py:41-42) or
    ``[N, out]`` for per-sample gradients (``grad_batch[n] = delta_n z_n^T``); ``z: [N, in]``.  Stored under the
    savefield in place of the tensor when an extension is created with ``factorised=True``: the only representation
    that exists at BASELINE config 5 (the tensor would be 2.7 TB).  ``vivit_amd.optim`` contracts it with two small
    GEMMs and the fused Hadamard kernel."""

    def __init__(self, s: Tensor, z: Tensor):
        self.s, self.z = s.contiguous(), z.contiguous()

    @property
    def shape(self):
        return tuple(self.s.shape) + (self.z.shape[1],)

    def dim(self):
        return self.s.dim() + 1

    def detach(self):
        return self

    def materialise(self) -> Tensor:
        """The explicit tensor (small problems / mixed representations only)."""
        if self.s.is_cuda and self.s.dtype == torch.float32:   # the HIP store-stream kernel of the weight rule
            if self.s.dim() == 2:
                return kernels.linear_weight_mjp(self.s.unsqueeze(0), self.z)[0]
            return kernels.linear_weight_mjp(self.s, self.z)
        if self.s.dim() == 2:
            return torch.einsum("no,ni->noi", self.s, self.z)
        return torch.einsum("cno,ni->cnoi", self.s, self.z)


class _Extension:
    savefield = None
    # Stream contract (backend/engine.py): an extension whose ``apply`` reads ``g_out`` (autograd's gradient) keeps
    # ``uses_grad = True`` -- the extensions' stream then waits for the backward pass at every hook and the gradient is
    # recorded on it.  Only extensions that provably ignore ``g_out`` (the sqrt-GGN family) may set it to False.
    uses_grad = True

    def __init__(self, subsampling: Optional[List[int]] = None):
        self._subsampling = subsampling

    def get_subsampling(self):
        return self._subsampling

    def apply(self, ctx, module, g_out):
        raise NotImplementedError


def _own_params(module):
    return [(name, p) for name, p in module._parameters.items() if p is not None and p.requires_grad]


def _spatial_sum(t: Tensor, keep: int) -> Tensor:
    """Sum all dims after the first ``keep`` ones (HIP: one wave per row, fixed order)."""
    if t.dim() <= keep:
        return t
    if t.is_cuda:
        lead = t.shape[:keep]
        return kernels.row_dot(t.reshape(-1, t[(0,) * keep].numel())).view(lead)
    return t.flatten(start_dim=keep).sum(keep)


def _spatial_sum3(M: Tensor) -> Tensor:
    """``_spatial_sum(M, 3)`` remembered ON the factor tensor: BatchNorm's bias rule and its weight rule both need it (one pass
    over M instead of two; the memo lives and dies with the tensor object)."""
    memo = getattr(M, "_vivit_ssum3", None)
    if memo is None:
        memo = _spatial_sum(M, 3)
        try:
            M._vivit_ssum3 = memo
        except AttributeError:   # (tensor subclasses without a __dict__)
            pass
    return memo


def _bn_constants(module):
    """``(rstd, scale)`` of a BatchNorm in eval mode, recomputed at every use (two tiny launches): the three rules of a module
    share them through the memo :func:`_bn_eval_rules` keeps on the factor tensor, i.e. for one backward pass.  Nothing is
    remembered on the module: writes through ``.data`` (``bn.weight.data = ...``, as the reference's tests re-initialise,
    test/utils.py:111) leave ``_version`` and ``data_ptr`` unchanged, so no key on the module can tell stale constants."""
    rstd = torch.rsqrt(module.running_var + module.eps)
    scale = rstd * module.weight.detach() if module.weight is not None else rstd
    return rstd, scale


def _bn_scale(module) -> Tensor:
    return _bn_constants(module)[1]


def _bn_eval_rules(module, M: Tensor, x: Tensor):
    """``(M scale_c, (sum_l M x - mean_c sum_l M) rstd_c, sum_l M)`` of a BatchNorm in eval mode from ONE pass over the factor ``M [V, N, C, *spatial]``
    (``vivit_bn_eval_rules_f32``), remembered on the tensor: the weight rule, the bias rule and the input rule of the module
    are three calls on the same ``M`` (round 4: three row reductions and one scaling pass, four reads of ``M``)."""
    memo = getattr(M, "_vivit_bn_rules", None)
    if memo is None or memo[0] is not module:
        Mc = M if M.dim() > 3 else M.unsqueeze(-1)
        xc = x if x.dim() > 2 else x.unsqueeze(-1)
        rstd, scale = _bn_constants(module)
        out, mx, ms = kernels.bn_eval_rules(Mc, xc, scale, module.running_mean, rstd)   # mx: the finished weight rule
        memo = (module, out.view(M.shape), mx, ms)
        try:
            M._vivit_bn_rules = memo
        except AttributeError:   # (tensor subclasses without a __dict__)
            pass
    return memo[1:]


def _norm_geometry(module, x: Tensor):
    """``(rows, G, S, A)`` of a LayerNorm / GroupNorm on the input ``x`` in the notation of csrc/norm_rules.hip: ``rows`` sets of
    contiguous elements that share one mean and variance, ``G`` groups of gamma indices, segments of ``S`` elements that share one
    gamma, ``A`` rows per sample."""
    if isinstance(module, nn.LayerNorm):
        rows = x.numel() // math.prod(module.normalized_shape)
        return rows, 1, 1, rows // x.shape[0]
    return x.shape[0] * module.num_groups, module.num_groups, math.prod(x.shape[2:]), module.num_groups


def _norm_rules(module, M: Tensor, x: Tensor, input_rule: bool):
    """``(input rule, weight rule, bias rule)`` of a LayerNorm / GroupNorm on the HIP kernels, remembered on the factor tensor as
    :func:`_bn_eval_rules` does: the rules of one module are up to three calls on the same ``M``.  The statistics are computed once
    (``vivit_norm_stats_f32``), then ONE launch visits every row of ``M`` for the input rule and the parameter rules that live
    inside a row (``vivit_norm_rules_f32``: GroupNorm's sums over the spatial positions, LayerNorm's ``M xhat``); a LayerNorm with
    extra dimensions sums over them in a launch of its own (``vivit_norm_position_sums_f32``).  Rules of parameters that are
    absent or frozen are not computed (``None``), the input rule only when ``input_rule`` says that it will be asked for.
    Nothing is remembered on the module."""
    memo = getattr(M, "_vivit_norm_rules", None)
    if memo is not None and memo[0] is module and (memo[1] is not None or not input_rule):
        return memo[1:]
    own = {name for name, _ in _own_params(module)}
    rows, G, S, A = _norm_geometry(module, x)
    gamma = module.weight.detach() if module.weight is not None else None
    mean, rstd = kernels.norm_stats(x, rows, module.eps)
    w = b = None
    if isinstance(module, nn.LayerNorm):
        shape = tuple(M.shape[:2]) + tuple(module.normalized_shape)
        if A == 1:     # the rows are the samples: the weight rule is elementwise, the bias rule is the factor itself
            out, w, _ = kernels.norm_rules(M, x, gamma, mean, rstd, want=(input_rule, "weight" in own, False))
            w = w.view(shape) if w is not None else None
            b = M.reshape(shape) if "bias" in own else None
        else:
            out = kernels.norm_rules(M, x, gamma, mean, rstd, want=(True, False, False))[0] if input_rule else None
            if own:
                D = math.prod(module.normalized_shape)
                w, b = (t.view(shape) for t in kernels.norm_position_sums(M.reshape(M.shape[0], M.shape[1], A, D), x.reshape(-1, A, D), mean, rstd))
    else:
        out, w, b = kernels.norm_rules(M, x, gamma, mean, rstd, G, S, want=(input_rule, "weight" in own, "bias" in own))
        w, b = (t.view(*M.shape[:2], module.num_channels) if t is not None else None for t in (w, b))
    memo = (module, out, w, b)
    try:
        M._vivit_norm_rules = memo
    except AttributeError:   # (tensor subclasses without a __dict__)
        pass
    return memo[1:]


def _norm_xhat(module, x: Tensor) -> Tensor:
    """The normalised input of a LayerNorm / GroupNorm without its affine part (plain torch: the rule of non-HIP tensors)."""
    if isinstance(module, nn.LayerNorm):
        return F.layer_norm(x, module.normalized_shape, None, None, module.eps)
    return F.group_norm(x, module.num_groups, None, None, module.eps)


def _rms_geometry(module, x: Tensor):
    """``(rows, A, eps)`` of an RMSNorm on the input ``x`` in the notation of csrc/llama_rules.hip: ``rows`` sets of ``L =
    prod(normalized_shape)`` contiguous elements that share one statistic, ``A`` rows per sample; ``eps=None`` is the machine
    epsilon of the input's dtype, as in ``F.rms_norm``."""
    rows = x.numel() // math.prod(module.normalized_shape)
    return rows, rows // x.shape[0], module.eps if module.eps is not None else torch.finfo(x.dtype).eps


def _rms_norm_rules(module, M: Tensor, x: Tensor, input_rule: bool):
    """``(input rule, weight rule)`` of an RMSNorm on the HIP kernels, remembered on the factor tensor as :func:`_norm_rules` does.
    ``rstd`` is computed once (``vivit_rms_norm_stats_f32``), then ONE launch visits every row of ``M`` for the input rule and --
    without extra dimensions -- the weight rule ``M xhat`` (``vivit_rms_norm_rules_f32``); with extra dimensions the weight rule sums
    over them in a launch of its own (``vivit_rms_norm_position_sums_f32``).  Nothing is computed for an absent or frozen weight
    (``None``), the input rule only when ``input_rule`` says that it will be asked for.  Nothing is remembered on the module."""
    memo = getattr(M, "_vivit_rms_norm_rules", None)
    if memo is not None and memo[0] is module and (memo[1] is not None or not input_rule):
        return memo[1:]
    own = bool(_own_params(module))
    rows, A, eps = _rms_geometry(module, x)
    gamma = module.weight.detach() if module.weight is not None else None
    out = w = None
    if input_rule or own:
        rstd = kernels.rms_norm_stats(x, rows, eps)
        shape = tuple(M.shape[:2]) + tuple(module.normalized_shape)
        if A == 1:     # the rows are the samples: the weight rule is elementwise
            out, w = kernels.rms_norm_rules(M, x, gamma, rstd, want=(input_rule, own))
            w = w.view(shape) if w is not None else None
        else:
            out = kernels.rms_norm_rules(M, x, gamma, rstd, want=(True, False))[0] if input_rule else None
            if own:
                D = math.prod(module.normalized_shape)
                w = kernels.rms_norm_position_sums(M.reshape(M.shape[0], M.shape[1], A, D), x.reshape(-1, A, D), rstd).view(shape)
    memo = (module, out, w)
    try:
        M._vivit_rms_norm_rules = memo
    except AttributeError:   # (tensor subclasses without a __dict__)
        pass
    return memo[1:]


def _rms_norm_jac_t_torch(module, M: Tensor, x: Tensor) -> Tensor:
    """The input rule of csrc/llama_rules.hip in plain torch (non-HIP or non-fp32 tensors): ``rstd (h - xhat mean(h xhat))``.  No
    autograd."""
    dims = tuple(range(-len(module.normalized_shape), 0))
    eps = _rms_geometry(module, x)[2]
    xhat = F.rms_norm(x, module.normalized_shape, None, eps)
    rstd = torch.rsqrt(x.pow(2).mean(dims, keepdim=True) + eps)
    h = M.reshape(M.shape[0], *x.shape)
    if module.weight is not None:
        h = h * module.weight.detach()
    return rstd * (h - xhat * (h * xhat).mean(dims, keepdim=True))


def _param_factor(module, name: str, M: Tensor, x: Tensor, subsampling=None) -> Tensor:
    """``param_mjp(..., sum_batch=False)``: ``M`` [V, N, *out] -> [V, N, *param.shape].  ``subsampling``: the indices ``x`` was
    sub-sampled with (a rule that reads what the forward pass left on the module sub-samples it likewise)."""
    if isinstance(module, nn.Linear):
        if name == "bias":
            return M if M.dim() == 3 else M.flatten(2, -2).sum(2)
        if M.dim() == 3:
            return kernels.linear_weight_mjp(M, x)           # "vno,ni->vnoi" (HIP store-stream kernel)
        return _linear_seq_weight_factor(M, x)
    if isinstance(module, _CONVS):
        if name == "bias":
            return _spatial_sum(M, 3)
        if (M.is_cuda and M.dtype == torch.float32 and isinstance(module.padding, tuple) and module.padding_mode == "zeros"):
            try:
                if isinstance(module, (nn.Conv3d, nn.ConvTranspose3d)):
                    return _hip_conv3d_weight_factor(module, M, x)
                return _hip_conv_weight_factor(module, M, x)
            except _lib.VivitHipError as exc:  # shapes outside the kernel's launch limits: the torch rule below
                if exc.status != _lib.VIVIT_E_UNSUPPORTED:
                    raise
        return _conv_weight_factor(module, M, x)
    if isinstance(module, _BATCHNORM):
        if module.training:
            raise NotImplementedError("BatchNorm must be in eval mode (as in the reference tests)")
        if M.is_cuda and M.dtype == torch.float32:
            # sum_l M xhat = (sum_l M x - mean_c sum_l M) rstd_c: both row reductions (and the input rule's scaling) come out of
            # one pass over M; the rest is [V, N, C]-sized
            _, Mw, Ms = _bn_eval_rules(module, M, x)
            return Ms if name == "bias" else Mw
        if name == "bias":
            return _spatial_sum3(M)
        rstd = torch.rsqrt(module.running_var + module.eps)
        shape = [1, -1] + [1] * (x.dim() - 2)
        xhat = (x - module.running_mean.view(shape)) * rstd.view(shape)
        return _spatial_sum(M * xhat.unsqueeze(0), 3)
    if isinstance(module, _NORMS):
        if M.is_cuda and M.dtype == torch.float32:
            # (the input rule rides the same visit of M when the back-propagation goes on below this module)
            _, Mw, Mb = _norm_rules(module, M, x, module.input0.requires_grad)
            return Mb if name == "bias" else Mw
        T = M if name == "bias" else M * _norm_xhat(module, x).unsqueeze(0)
        if isinstance(module, nn.LayerNorm):   # weight [*D]: the extra dimensions between batch and D are summed
            extra = tuple(range(2, M.dim() - len(module.normalized_shape)))
            return T.sum(extra) if extra else T
        return T.flatten(3).sum(3) if T.dim() > 3 else T
    if isinstance(module, nn.RMSNorm):   # weight [*D] only
        if M.is_cuda and M.dtype == torch.float32:
            # (the input rule rides the same visit of M when the back-propagation goes on below this module)
            return _rms_norm_rules(module, M, x, module.input0.requires_grad)[1]
        T = M.reshape(M.shape[0], *x.shape) * F.rms_norm(x, module.normalized_shape, None, _rms_geometry(module, x)[2]).unsqueeze(0)
        extra = tuple(range(2, T.dim() - len(module.normalized_shape)))   # the extra dimensions between batch and D are summed
        return T.sum(extra) if extra else T
    if isinstance(module, nn.Embedding):
        B, ids = _embedding_compact(module, M, x)
        return _embedding_factor(B, ids, module.num_embeddings)
    if isinstance(module, ScaledDotProductAttention) and name == "bias":   # a learned relative-position table
        return _attention_bias_factor(module, M, x, subsampling)
    raise NotImplementedError(f"no parameter rule for {type(module).__name__}")


def _param_factor_of(module, name: str, M: Tensor, x: Tensor, subsampling) -> Tensor:
    """:func:`_param_factor` as the extensions call it: the sub-sampling goes to the one rule that reads what the forward pass left on
    the module (the attention leaf's table); every other rule is called with the four arguments it always had."""
    if isinstance(module, ScaledDotProductAttention):
        return _param_factor(module, name, M, x, subsampling=subsampling)
    return _param_factor(module, name, M, x)


def _linear_seq_weight_factor(M: Tensor, x: Tensor) -> Tensor:
    """The explicit weight factor ``[V, N, O, I]`` of a Linear on ``x [N, *A, I]`` from ``M [V, N, *A, O]``."""
    Ma, xa = M.flatten(2, -2), x.flatten(1, -2)              # [V, N, A, O], [N, A, I]  (linear.py:52-81: extra dims are summed)
    if M.is_cuda and M.dtype == torch.float32:
        # a 1 x 1 convolution over the A positions: the HIP weight rule of the convolution, "vnoa,nia->vnoi"
        out = kernels.conv2d_weight_mjp(Ma.transpose(2, 3).unsqueeze(3).contiguous(), xa.transpose(1, 2).unsqueeze(2).contiguous(),
                                        (1, 1), (1, 1), (0, 0), (1, 1))
        return out.reshape(out.shape[:4])
    return torch.einsum("vnao,nai->vnoi", Ma, xa)


def _embedding_compact(module, M: Tensor, idx: Tensor):
    """Compact form ``(B [V, N, T, D], ids [N, T])`` of an Embedding's weight factor ``Vt[v, n, w] = sum_{t: idx[n, t] = w} M[v, n, t]``
    (csrc/embedding.hip): sample n's distinct tokens in increasing order, then -1, and the rows of ``M [V, N, *, D]`` summed per token;
    positions with ``idx == padding_idx`` contribute nothing.  Extra input dimensions are flattened into ``T``.  HIP fp32 tensors:
    ``kernels.embedding_compact``; any other tensor: the same in plain torch (``index_add_``)."""
    if module.max_norm is not None:        # the forward rewrites the weights
        raise NotImplementedError("nn.Embedding with max_norm is not supported by the stand-in backend")
    if module.scale_grad_by_freq:          # the gradient is rescaled per token
        raise NotImplementedError("nn.Embedding with scale_grad_by_freq is not supported by the stand-in backend")
    if idx.is_floating_point():
        raise ValueError(f"nn.Embedding expects integer token ids, got {idx.dtype}")
    V, N, D = M.shape[0], idx.shape[0], module.embedding_dim
    M, idx = M.reshape(V, N, -1, D), idx.reshape(N, -1)
    if M.is_cuda and M.dtype == torch.float32:
        return kernels.embedding_compact(M, idx, module.padding_idx)
    T = idx.shape[1]
    ids, _, _, _, slot_of_t = kernels.embedding_token_slots(idx, module.padding_idx)
    dest = slot_of_t + (T + 1) * torch.arange(N, device=idx.device).unsqueeze(1)     # padding positions go to a spare slot T
    B = M.new_zeros((V, N * (T + 1), D)).index_add_(1, dest.reshape(-1), M.reshape(V, N * T, D))
    return B.view(V, N, T + 1, D)[:, :, :T].contiguous(), ids


def _embedding_factor(B: Tensor, ids: Tensor, W: int) -> Tensor:
    """The explicit factor ``[V, N, W, D]`` from the compact form: zeros plus the rows ``B[v, n, u]`` at ``ids[n, u]``."""
    if B.is_cuda and B.dtype == torch.float32:
        return kernels.embedding_weight_mjp(B, ids, W)
    V, N, T, D = B.shape
    dest = ids.to(torch.int64).masked_fill(ids < 0, W) + (W + 1) * torch.arange(N, device=ids.device).unsqueeze(1)
    out = B.new_zeros((V, N * (W + 1), D)).index_add_(1, dest.reshape(-1), B.reshape(V, N * T, D))
    return out.view(V, N, W + 1, D)[:, :, :W].contiguous()


_CONV_FN = {nn.Conv1d: F.conv1d, nn.Conv2d: F.conv2d, nn.Conv3d: F.conv3d, nn.ConvTranspose1d: F.conv_transpose1d,
            nn.ConvTranspose2d: F.conv_transpose2d, nn.ConvTranspose3d: F.conv_transpose3d}


def _hip_conv_weight_factor(module, M: Tensor, x: Tensor) -> Tensor:
    """Weight rule of Conv1d/2d and ConvTranspose1d/2d (any ``groups``, zero padding) on ONE HIP kernel
    (csrc/jacobians.hip: unfold + "vnol,nkl->vnok", patch values gathered on the fly, no im2col buffer).

    * a 1-D convolution is the 2-D one with a single row;
    * ``groups > 1``: one launch per group on the group's channel slices (the weight's leading axis is the groups'
      output channels one after the other -- convnd.py:9-30 through BackPACK's grouped unfold);
    * a transposed convolution y = conv_transpose(x, W) is the adjoint of a convolution with the same stride / padding /
      dilation, so dL/dW[ci, co, k] = sum_q x[ci, q] M[co, q s - p + k d] is the SAME contraction with the roles swapped:
      ``M`` is the image the patches are gathered from, ``x`` the coefficient (convtransposend.py:9-30).  The kernel
      gathers from the operand without a slice axis, so the slice axis of ``M`` is folded into the batch and ``x`` is
      repeated over it."""
    one_d = isinstance(module, (nn.Conv1d, nn.ConvTranspose1d))
    transposed = isinstance(module, (nn.ConvTranspose1d, nn.ConvTranspose2d))
    if one_d:
        M, x = M.unsqueeze(3), x.unsqueeze(2)
        ks, st, pd, dl = (1, module.kernel_size[0]), (1, module.stride[0]), (0, module.padding[0]), (1, module.dilation[0])
    else:
        ks, st, pd, dl = module.kernel_size, module.stride, module.padding, module.dilation
    V, N, G = M.shape[0], M.shape[1], module.groups
    if transposed:
        coef = x.unsqueeze(0).expand(V, *x.shape).reshape(1, V * N, *x.shape[1:])     # [1, V N, Cin, Hq, Wq]
        image = M.reshape(V * N, *M.shape[2:])                                         # [V N, Cout, H', W']
    else:
        coef, image = M, x
    Cc, Ci = coef.shape[2] // G, image.shape[1] // G
    parts = []
    for g in range(G):
        c = coef if G == 1 else coef[:, :, g * Cc:(g + 1) * Cc]
        im = image if G == 1 else image[:, g * Ci:(g + 1) * Ci]
        parts.append(kernels.conv2d_weight_mjp(c.contiguous(), im.contiguous(), ks, st, pd, dl))
    out = parts[0] if G == 1 else torch.cat(parts, 2)     # [.., .., coefficient channels, image channels / G, kh, kw]
    if transposed:
        out = out.view(V, N, *out.shape[2:])
    return out.squeeze(4) if one_d else out


def _triple(v):
    return (v, v, v) if isinstance(v, int) else tuple(v)


def _depth_range(n_out: int, n_in: int, s: int, p: int, off: int):
    """Positions ``q`` in ``[0, n_out)`` whose partner ``q s - p + off`` lies in ``[0, n_in)``: ``(q_lo, q_hi, first partner)``
    (``q_hi < q_lo``: none)."""
    q_lo = max(0, -((off - p) // s))            # ceil((p - off) / s)
    q_hi = min(n_out - 1, (n_in - 1 + p - off) // s)
    return q_lo, q_hi, q_lo * s - p + off


def _conv3d_weight_contract(coef: Tensor, image: Tensor, ks, st, pd, dl) -> Tensor:
    """``out[v, n, c, i, kd, kh, kw] = sum_q coef[v, n, c, qd, qh, qw] image[n, i, qd sd - pd + kd dd, qh sh - ph + kh dh,
    qw sw - pw + kw dw]`` -- the weight rule of a three-dimensional convolution -- on the TWO-dimensional HIP kernel, one
    launch per depth tap ``kd``: the depth slices are stacked along the height of one tall image.  Behind each coefficient
    slice stand ``ceil((KH - 1) dh / sh)`` zero rows, so that a window that starts in a slice's last rows and runs into the
    next slice meets a zero coefficient; the image slices carry their height padding explicitly at the matching pitch.
    ``coef: [V, N, C, QD, QH, QW]``, ``image: [N, I, D, H, W]`` -> ``[V, N, C, I, KD, KH, KW]``."""
    Vc, Nc, Cc, QD, QH, QW = coef.shape
    _, Ci, D, H, W = image.shape
    (KD, KH, KW), (sd, sh, sw), (pdd, ph, pw), (dd, dh, dw) = ks, st, pd, dl
    extra = -(-((KH - 1) * dh) // sh)
    QHp = QH + extra
    Hp = QHp * sh                      # pitch of an image slice: window row qh sh + kh dh of slice qd is row qd Hp + ...
    tail = (KH - 1) * dh               # rows behind the last slice that windows of (zero) coefficient rows still address
    cs = coef.new_zeros((Vc, Nc, Cc, QD, QHp, QW))
    cs[..., :QH, :] = coef
    cs = cs.view(Vc, Nc, Cc, QD * QHp, QW)
    hrows = min(H, Hp - ph)            # image rows that fall inside a slice (the rest is never read by a live window)
    outs = []
    for kd in range(KD):
        xs = image.new_zeros((Nc, Ci, QD * Hp + tail, W))
        q_lo, q_hi, d_lo = _depth_range(QD, D, sd, pdd, kd * dd)
        if q_hi >= q_lo and hrows > 0:
            nq = q_hi - q_lo + 1
            xv = xs[:, :, :QD * Hp].view(Nc, Ci, QD, Hp, W)
            xv[:, :, q_lo:q_hi + 1, ph:ph + hrows] = image[:, :, d_lo:d_lo + (nq - 1) * sd + 1:sd, :hrows]
        outs.append(kernels.conv2d_weight_mjp(cs, xs, (KH, KW), (sh, sw), (0, pw), (dh, dw)))
    return torch.stack(outs, 4)


def _hip_conv3d_weight_factor(module, M: Tensor, x: Tensor) -> Tensor:
    """Weight rule of Conv3d / ConvTranspose3d (any ``groups``, zero padding; convnd.py:25-30, convtransposend.py:25-30)
    on the HIP kernel of the two-dimensional rule (:func:`_conv3d_weight_contract`).  As in two dimensions, the transposed
    convolution's rule is the same contraction with the roles of factor and input swapped, and a grouped layer is one
    contraction per group on its channel slices."""
    transposed = isinstance(module, nn.ConvTranspose3d)
    ks, st, pd, dl = module.kernel_size, module.stride, module.padding, module.dilation
    V, N, G = M.shape[0], M.shape[1], module.groups
    if transposed:
        coef = x.unsqueeze(0).expand(V, *x.shape).reshape(1, V * N, *x.shape[1:])     # [1, V N, Cin, Dq, Hq, Wq]
        image = M.reshape(V * N, *M.shape[2:])                                         # [V N, Cout, D', H', W']
    else:
        coef, image = M, x
    Cc, Ci = coef.shape[2] // G, image.shape[1] // G
    parts = []
    for g in range(G):
        c = coef if G == 1 else coef[:, :, g * Cc:(g + 1) * Cc]
        im = image if G == 1 else image[:, g * Ci:(g + 1) * Ci]
        parts.append(_conv3d_weight_contract(c, im, ks, st, pd, dl))
    out = parts[0] if G == 1 else torch.cat(parts, 2)
    return out.view(V, N, *out.shape[2:]) if transposed else out


def _hip_conv3d_jac_t(module, M: Tensor, x: Tensor) -> Tensor:
    """Input rule of Conv3d (any ``groups``, zero padding) on the two-dimensional HIP kernel: for every depth tap ``kd`` the
    output slices ``od`` are a batch of two-dimensional problems whose results are added into the input slices
    ``d = od sd - pd + kd dd`` (for a fixed tap that map is one strided slice)."""
    W = module.weight.detach()
    (KD, KH, KW), (sd, sh, sw), (pdd, ph, pw), (dd, dh, dw) = module.kernel_size, module.stride, module.padding, module.dilation
    V, N, Cout, OD, OH, OW = M.shape
    _, Cin, D, H, Wd = x.shape
    G = module.groups
    Co, Ci = Cout // G, Cin // G
    Mt = M.permute(0, 1, 3, 2, 4, 5).reshape(V, N * OD, Cout, OH, OW)
    g = M.new_zeros((V, N, Cin, D, H, Wd))
    for kd in range(KD):
        o_lo, o_hi, d_lo = _depth_range(OD, D, sd, pdd, kd * dd)
        if o_hi < o_lo:
            continue
        Wk = W[:, :, kd]
        if G == 1:
            res = kernels.conv2d_jac_t(Mt, Wk, (H, Wd), (sh, sw), (ph, pw), (dh, dw))
        else:
            res = torch.cat([kernels.conv2d_jac_t(Mt[:, :, i * Co:(i + 1) * Co].contiguous(), Wk[i * Co:(i + 1) * Co].contiguous(),
                                                  (H, Wd), (sh, sw), (ph, pw), (dh, dw)) for i in range(G)], 2)
        res = res.view(V, N, OD, Cin, H, Wd)[:, :, o_lo:o_hi + 1].permute(0, 1, 3, 2, 4, 5)
        g[:, :, :, d_lo:d_lo + (o_hi - o_lo) * sd + 1:sd] += res
    return g


def _hip_convtranspose3d_jac_t(module, M: Tensor, x: Tensor) -> Optional[Tensor]:
    """Input rule of ConvTranspose3d: a forward convolution of ``M`` with the weight,
    ``g[ci, q] = sum_{co, k} W[ci, co, k] M[co, q s - p + k d]`` -- per depth tap ``kd`` the two-dimensional rule of
    :func:`_convtranspose2d_input` on the slices ``M[.., qd sd - pd + kd dd]`` (a batch), summed over the taps."""
    W = module.weight.detach()
    (KD, KH, KW), (sd, sh, sw), (pdd, ph, pw), (dd, dh, dw) = module.kernel_size, module.stride, module.padding, module.dilation
    V, N, Cout, Dm, Hm, Wm = M.shape
    _, Cin, QD, QH, QW = x.shape
    g = M.new_zeros((V, N, Cin, QD, QH, QW))
    for kd in range(KD):
        q_lo, q_hi, d_lo = _depth_range(QD, Dm, sd, pdd, kd * dd)
        if q_hi < q_lo:
            continue
        nq = q_hi - q_lo + 1
        Mk = M[:, :, :, d_lo:d_lo + (nq - 1) * sd + 1:sd].permute(0, 1, 3, 2, 4, 5).reshape(V, N * nq, Cout, Hm, Wm)
        res = _convtranspose2d_input(Mk, W[:, :, kd], (KH, KW), (sh, sw), (ph, pw), (dh, dw), module.groups, (QH, QW))
        if res is None:
            return None
        g[:, :, :, q_lo:q_hi + 1] += res.view(V, N, nq, Cin, QH, QW).permute(0, 1, 3, 2, 4, 5)
    return g


def _hip_pool3d_jac_t(module, M: Tensor, x: Tensor) -> Optional[Tensor]:
    """MaxPool3d / AvgPool3d on the two-dimensional pooling kernels.  Both poolings are separable -- a window over
    (d, h, w) is a window over (h, w) in every depth slice followed by a window over d -- and so are their Jacobians:
    the depth stage is the two-dimensional kernel on the image ``[D, OH * OW]`` with a ``(kd, 1)`` window.  For the
    maximum the composition selects the same element as the three-dimensional scan (first maximum in d-major order),
    and -inf padding composes; the average (count_include_pad) divides by kh kw and then by kd."""
    V, N, C, OD, OH, OW = M.shape
    _, _, D, H, W = x.shape
    ks = _triple(module.kernel_size)
    st = _triple(module.stride if module.stride is not None else module.kernel_size)
    pd = _triple(module.padding)
    if isinstance(module, nn.MaxPool3d):
        if _triple(module.dilation) != (1, 1, 1) or module.ceil_mode or module.return_indices:
            return None
        x2 = x.reshape(N, C * D, H, W)
        y1 = F.max_pool2d(x2, ks[1:], st[1:], pd[1:])                                   # the in-plane maxima (forward values only)
        g1 = kernels.maxpool2d_jac_t(M.reshape(V, N, C, OD, OH * OW), y1.reshape(N, C, D, OH * OW), (ks[0], 1), (st[0], 1), (pd[0], 0))
        return kernels.maxpool2d_jac_t(g1.reshape(V, N, C * D, OH, OW), x2, ks[1:], st[1:], pd[1:]).view(V, N, C, D, H, W)
    if module.ceil_mode or not module.count_include_pad or module.divisor_override is not None:
        return None
    g1 = kernels.avgpool2d_jac_t(M.reshape(V, N, C, OD, OH * OW), (D, OH * OW), (ks[0], 1), (st[0], 1), (pd[0], 0))
    return kernels.avgpool2d_jac_t(g1.reshape(V, N, C * D, OH, OW), (H, W), ks[1:], st[1:], pd[1:]).view(V, N, C, D, H, W)


def _conv_weight_factor(module, M: Tensor, x: Tensor) -> Tensor:
    """Weight rule of the convolution family (Conv1d/3d, grouped Conv2d, ConvTranspose1d/2d/3d; the derivative classes
    of vivit/extensions/secondorder/vivit/convnd.py:9-30 and convtransposend.py:9-30): per sample ``n`` and slice ``v``
    the vector-Jacobian product of the functional convolution w.r.t. its weight, batched with ``torch.func.vmap``."""
    from torch.func import vjp, vmap

    fn = _CONV_FN[type(module)]
    kw = dict(stride=module.stride, padding=module.padding, dilation=module.dilation, groups=module.groups)
    if isinstance(module, (nn.ConvTranspose1d, nn.ConvTranspose2d, nn.ConvTranspose3d)):
        kw["output_padding"] = module.output_padding
    if getattr(module, "padding_mode", "zeros") != "zeros":
        raise NotImplementedError("only zero padding is supported by the stand-in backend")
    weight = module.weight.detach()

    def single(xn, mvn):  # xn: [*in], mvn: [*out]
        _, pull = vjp(lambda w: fn(xn.unsqueeze(0), w, None, **kw).squeeze(0), weight)
        return pull(mvn)[0]

    return vmap(vmap(single, in_dims=(0, 0)), in_dims=(None, 0))(x, M)


_ACTIVATIONS = {nn.ReLU: ("relu", None), nn.Sigmoid: ("sigmoid", None), nn.Tanh: ("tanh", None),
                nn.LeakyReLU: ("leaky_relu", "negative_slope"), nn.LogSigmoid: ("logsigmoid", None), nn.ELU: ("elu", "alpha"),
                nn.SELU: ("selu", None), nn.GELU: ("gelu", None), nn.SiLU: ("silu", None),   # (GELU: see _activation_kind)
                SoftCap: ("softcap", "cap")}


def _activation_kind(module):
    """``(kind of kernels.act_jac_t, parameter)`` of an activation module, ``None`` for any other module."""
    kind = _ACTIVATIONS.get(type(module))
    if kind is None:
        return None
    if isinstance(module, nn.GELU) and module.approximate == "tanh":
        return "gelu_tanh", 0.0
    return kind[0], getattr(module, kind[1]) if kind[1] else 0.0


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _single(v):
    return v if isinstance(v, int) else tuple(v)[0]


def _attention_out(module, x: Tensor, subsampling) -> Tensor:
    """The forward output of a :class:`ScaledDotProductAttention` for the samples of ``x``: what the forward pass left on the module,
    sub-sampled as ``x`` was (repeated indices repeat rows).  Only a module that was called outside the engine has none: one forward.
    An output that does not belong to ``x`` (samples, tokens, device or dtype) is an error, never a second forward."""
    out = getattr(module, "output", None)
    if out is None:
        with torch.no_grad():
            return module.attend(x, _attention_lengths(module, x, subsampling))
    out = subsample(out.detach(), 0, subsampling)
    want = (*x.shape[:2], module.head_dim(x) * module.num_heads)   # the output has H d columns
    if tuple(out.shape) != want or out.device != x.device or out.dtype != x.dtype:
        raise ValueError(f"ScaledDotProductAttention: module.output {tuple(out.shape)} {out.dtype} on {out.device} after sub-sampling "
                         f"does not belong to the input {tuple(x.shape)} {x.dtype} on {x.device} (expected {want})")
    return out


def _attention_lengths(module, x: Tensor, subsampling) -> Optional[Tensor]:
    """The lengths the forward pass of a :class:`ScaledDotProductAttention` used (int32 ``[N]``, kept on the module), sub-sampled as
    ``x`` was; ``None``: that pass had none."""
    lengths = getattr(module, "forward_lengths", None)
    if lengths is None:
        return None
    lengths = subsample(lengths, 0, subsampling).to(x.device)
    if lengths.shape[0] != x.shape[0]:
        raise ValueError(f"ScaledDotProductAttention: the forward pass used {lengths.shape[0]} lengths after sub-sampling, the input "
                         f"has {x.shape[0]} samples")
    return lengths


def _attention_ds_torch(module, M: Tensor, x: Tensor, out: Tensor, lengths: Optional[Tensor]):
    """What the input rule and the table's rule share, in plain torch: the sizes, the operands split into heads, the logits ``Z`` before
    the score modifiers, ``P``, ``dO`` and ``dS = P (dP - D)`` ``[V, N, Hkv, R, T, T]``.  No autograd (the table is read detached)."""
    d, H, Hkv = module.head_dim(x), module.num_heads, module.kv_heads
    scale, R = module.scale_for(d), H // Hkv
    V, (N, T) = M.shape[0], x.shape[:2]
    M = M.reshape(V, N, T, H * d)
    hidden, dead = module.masks(T, lengths, x.device)
    if dead is not None:   # whatever the dead positions hold is not used
        M, x, out = M.masked_fill(dead, 0.0), x.masked_fill(dead, 0.0), out.masked_fill(dead, 0.0)
    q, k, v = _gqa_split(x, H, Hkv, d)                                             # q [N, Hkv, R, T, d]; k, v [N, Hkv, 1, T, d]
    Z = (q @ k.transpose(-1, -2)) * scale
    with torch.no_grad():
        S = module.modify(Z)
    if hidden is not None:
        S = S.masked_fill(hidden, float("-inf"))
    P = S.softmax(-1)                                                             # [N, Hkv, R, T, T], shared by the V slices
    dO = M.reshape(V, N, T, Hkv, R, d).permute(0, 1, 3, 4, 2, 5)                  # [V, N, Hkv, R, T, d]
    D = (dO * out.view(N, T, Hkv, R, d).permute(0, 2, 3, 1, 4)).sum(-1, keepdim=True)
    dS = P * (dO @ v.transpose(-1, -2) - D)
    return d, H, Hkv, scale, R, V, N, T, dead, q, k, Z, P, dO, dS


def _attention_bias_factor_torch(module, M: Tensor, x: Tensor, out: Tensor, lengths: Optional[Tensor] = None) -> Tensor:
    """The factor of a learned bias table in plain torch (non-HIP or non-fp32 tensors, head dimensions above 128): ``M [V, N, T, H d]``
    -> ``[V, N, *module.bias.shape]``, column ``b`` the sum of ``dS`` over the visible pairs whose distance reads column ``b`` of the
    table (``module.bias_columns``).  The table sits behind the cap: it is ``dS`` that is summed, not ``dZ``.  The sums over the
    diagonals are one reduction of a skewed view, the distances go to their columns through a product with a one-hot matrix: no
    scatter with atomics, the bytes are a function of the operands.  No autograd."""
    _, H, _, _, _, V, N, T, _, _, _, _, _, _, dS = _attention_ds_torch(module, M, x, out, lengths)
    # row i' = T - 1 - i of the flipped tile, padded to 2 T columns and re-read with 2 T - 1 columns, has entry (i, j) in column
    # i' + j = j - i + T - 1
    skew = F.pad(dS.reshape(V, N, H, T, T).flip(-2), (0, T)).flatten(-2)[..., :T * (2 * T - 1)].view(V, N, H, T, 2 * T - 1)
    diag = skew.sum(-2)                                                            # [V, N, H, 2 T - 1], by distance
    onehot = F.one_hot(module.bias_columns(T, x.device).long(), module.bias.shape[1]).to(diag.dtype)   # [2 T - 1, width]
    return diag @ onehot


def _attention_bias_factor(module, M: Tensor, x: Tensor, subsampling) -> Tensor:
    """The factor ``[V, N, *bias.shape]`` of the learned table of a :class:`ScaledDotProductAttention`: the kernel for HIP fp32 tensors
    with ``d <= 128`` (sizes beyond its index arithmetic come back as VIVIT_E_UNSUPPORTED), the same formula in torch otherwise.  The
    forward output and the lengths are those of the forward pass, sub-sampled as ``x`` was."""
    d, T = module.head_dim(x), x.shape[1]
    lengths, out = _attention_lengths(module, x, subsampling), _attention_out(module, x, subsampling)
    if M.is_cuda and M.dtype == torch.float32 and x.dtype == torch.float32 and d <= 128:
        try:
            return kernels.attention_bias_factor(M.reshape(M.shape[0], *x.shape[:2], -1), x, out, module.num_heads, module.scale_for(d),
                                                 module.causal, module.bias_for(T).detach().to(torch.float32).contiguous(),
                                                 index=module.bias_columns(T, x.device), width=module.bias.shape[1],
                                                 num_kv_heads=module.kv_heads, lengths=lengths, window=module.window,
                                                 softcap=module.softcap)
        except _lib.VivitHipError as exc:   # a shape beyond the kernel's launch limits: the formula below
            if exc.status != _lib.VIVIT_E_UNSUPPORTED:
                raise
    return _attention_bias_factor_torch(module, M, x, out, lengths)


def _attention_jac_t_torch(module, M: Tensor, x: Tensor, out: Tensor, lengths: Optional[Tensor] = None) -> Tensor:
    """The rule of csrc/attention.hip in plain torch (non-HIP or non-fp32 tensors): ``M [V, N, T, H d]``, ``x [N, T, (H + 2 Hkv) d]``,
    ``out [N, T, H d]`` -> ``[V, N, T, (H + 2 Hkv) d]``.  Query head ``h`` uses key / value head ``h // R``; dK and dV of a group are
    the sums over its ``R = H / Hkv`` query heads (multi-head attention: ``R = 1``).  K and V are broadcast views over the group axis,
    never expanded copies.  ``lengths`` (int32 ``[N]`` or ``None``) and ``module.window``: the mask of the forward pass; the rows of
    the dead positions are exact zeros.  ``module.softcap`` and ``module.bias``: the score function of the forward pass
    (``module.modify``), and ``dZ = dS (1 - t^2)`` in the place of ``dS`` under a cap.  No autograd."""
    d, H, Hkv, scale, R, V, N, T, dead, q, k, Z, P, dO, dS = _attention_ds_torch(module, M, x, out, lengths)
    if module.softcap is not None:   # dZ: the cap's derivative 1 - t^2, t = tanh(z / c)
        dS = dS * (1.0 - torch.tanh(Z / module.softcap) ** 2)
    dQ = (dS @ k) * scale                                                         # [V, N, Hkv, R, T, d]
    # the sum over the group's heads and over the queries is one contraction of length R T
    dV = P.reshape(N, Hkv, R * T, T).transpose(-1, -2) @ dO.reshape(V, N, Hkv, R * T, d)
    dK = (dS.reshape(V, N, Hkv, R * T, T).transpose(-1, -2) @ q.reshape(N, Hkv, R * T, d)) * scale
    G = torch.cat((dQ.permute(0, 1, 4, 2, 3, 5).reshape(V, N, T, H * d), dK.permute(0, 1, 3, 2, 4).reshape(V, N, T, Hkv * d),
                   dV.permute(0, 1, 3, 2, 4).reshape(V, N, T, Hkv * d)), -1)
    return G if dead is None else G.masked_fill(dead, 0.0)   # (a dead query saw itself: P = 1 on zeros; the sign of a zero)


def _cross_attention_lengths(module, q: Tensor, subsampling) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    """The query and key lengths the forward pass of a :class:`ScaledDotProductCrossAttention` used (int32 ``[N]``, kept on the
    module), sub-sampled as ``q`` was; ``None`` for a side that had none."""
    both = []
    for name in ("forward_query_lengths", "forward_key_lengths"):
        lengths = getattr(module, name, None)
        if lengths is not None:
            lengths = subsample(lengths, 0, subsampling).to(q.device)
            if lengths.shape[0] != q.shape[0]:
                raise ValueError(f"ScaledDotProductCrossAttention: the forward pass used {lengths.shape[0]} {name[8:]} after "
                                 f"sub-sampling, the input has {q.shape[0]} samples")
        both.append(lengths)
    return both[0], both[1]


def _cross_attention_out(module, q: Tensor, kv: Tensor, lengths, subsampling) -> Tensor:
    """The forward output of a :class:`ScaledDotProductCrossAttention` for the samples of ``q``, as :func:`_attention_out`: an output
    that does not belong to the inputs (samples, queries, device or dtype) is an error, never a second forward."""
    out = getattr(module, "output", None)
    if out is None:
        with torch.no_grad():
            return module.attend(q, kv, *lengths)
    out = subsample(out.detach(), 0, subsampling)
    if tuple(out.shape) != tuple(q.shape) or out.device != q.device or out.dtype != q.dtype:
        raise ValueError(f"ScaledDotProductCrossAttention: module.output {tuple(out.shape)} {out.dtype} on {out.device} after "
                         f"sub-sampling does not belong to the queries {tuple(q.shape)} {q.dtype} on {q.device}")
    return out


def _cross_attention_jac_t_torch(module, M: Tensor, q: Tensor, kv: Tensor, out: Tensor, query_lengths: Optional[Tensor] = None,
                                 key_lengths: Optional[Tensor] = None, want=(True, True)):
    """The rule of ``vivit_attention_cross_jac_t_f32`` in plain torch (non-HIP or non-fp32 tensors, head dimensions above 128):
    ``M [V, N, Tq, H d]``, ``q [N, Tq, H d]``, ``kv [N, Tk, 2 Hkv d]``, ``out [N, Tq, H d]`` -> ``(Gq [V, N, Tq, H d] | None,
    Gkv [V, N, Tk, 2 Hkv d] | None)`` as ``want`` says.  K and V are broadcast views over the group axis, never expanded copies;
    the rows of the dead positions (the module's docstring) are exact zeros.  No autograd."""
    d, H, Hkv = module.head_dim(q, kv), module.num_heads, module.kv_heads
    scale, R = module.scale_for(d), H // Hkv
    V, (N, Tq), Tk = M.shape[0], q.shape[:2], kv.shape[1]
    M = M.reshape(V, N, Tq, H * d)
    hidden, dead_q, dead_k = module.masks(N, Tq, Tk, query_lengths, key_lengths, q.device)
    if hidden is not None:   # whatever the dead positions hold is not used
        M, q, out, kv = M.masked_fill(dead_q, 0.0), q.masked_fill(dead_q, 0.0), out.masked_fill(dead_q, 0.0), kv.masked_fill(dead_k, 0.0)
    qh, k, v = module.split(q, kv, d)                                             # qh [N, Hkv, R, Tq, d]; k, v [N, Hkv, 1, Tk, d]
    S = (qh @ k.transpose(-1, -2)) * scale
    if hidden is not None:
        S = S.masked_fill(hidden, float("-inf"))
    P = S.softmax(-1)                                                             # [N, Hkv, R, Tq, Tk], shared by the V slices
    dO = M.reshape(V, N, Tq, Hkv, R, d).permute(0, 1, 3, 4, 2, 5)                 # [V, N, Hkv, R, Tq, d]
    D = (dO * out.reshape(N, Tq, Hkv, R, d).permute(0, 2, 3, 1, 4)).sum(-1, keepdim=True)
    dS = P * (dO @ v.transpose(-1, -2) - D)                                       # (a dead query saw key 0: P = 1 times dO = 0)
    Gq = Gkv = None
    if want[0]:
        Gq = ((dS @ k) * scale).permute(0, 1, 4, 2, 3, 5).reshape(V, N, Tq, H * d)
        if dead_q is not None:
            Gq = Gq.masked_fill(dead_q, 0.0)                                      # (the sign of a zero)
    if want[1]:   # the sum over the group's heads and over the queries is one contraction of length R Tq
        dV = P.reshape(N, Hkv, R * Tq, Tk).transpose(-1, -2) @ dO.reshape(V, N, Hkv, R * Tq, d)
        dK = (dS.reshape(V, N, Hkv, R * Tq, Tk).transpose(-1, -2) @ qh.reshape(N, Hkv, R * Tq, d)) * scale
        Gkv = torch.cat((dK.permute(0, 1, 3, 2, 4).reshape(V, N, Tk, Hkv * d), dV.permute(0, 1, 3, 2, 4).reshape(V, N, Tk, Hkv * d)), -1)
        if dead_k is not None:
            Gkv = Gkv.masked_fill(dead_k, 0.0)
    return Gq, Gkv


def _cross_attention_jac_t(module, M: Tensor, subsampling, want):
    """``(Gq | None, Gkv | None)``: the factor ``M [V, N, Tq, H d]`` at the output of a :class:`ScaledDotProductCrossAttention` taken
    to its two inputs -- the kernel for HIP fp32 tensors with head dimensions up to 128 (sizes beyond its index arithmetic come back
    as VIVIT_E_UNSUPPORTED), the same formula in torch for everything else."""
    q, kv = (subsample(t.detach(), 0, subsampling) for t in module.inputs)
    d = module.head_dim(q, kv)
    lengths = _cross_attention_lengths(module, q, subsampling)
    out = _cross_attention_out(module, q, kv, lengths, subsampling)
    M = M.reshape(M.shape[0], *q.shape[:2], -1)
    if M.is_cuda and M.dtype == torch.float32 and d <= 128:
        try:
            return kernels.cross_attention_jac_t(M, q, kv, out, module.num_heads, module.scale_for(d), num_kv_heads=module.kv_heads,
                                                 query_lengths=lengths[0], key_lengths=lengths[1], want=want)
        except _lib.VivitHipError as exc:
            if exc.status != _lib.VIVIT_E_UNSUPPORTED:
                raise
    return _cross_attention_jac_t_torch(module, M, q, kv, out, *lengths, want=want)


def _rope_jac_t_torch(module, M: Tensor, x: Tensor) -> Tensor:
    """The rule of ``vivit_rope_gqa_jac_t_f32`` in plain torch (non-HIP or non-fp32 tensors): the transposed rotation on the
    ``H + Hkv`` heads of the q and k parts of ``M [V, N, T, (H + 2 Hkv) d]`` with the tables of the forward pass, the ``Hkv d`` columns
    of v as they are.  No autograd."""
    d, rotated = module.head_dim(x), module.num_heads + module.kv_heads
    V, (N, T), half = M.shape[0], x.shape[:2], d // 2
    cos, sin = (t.view(1, 1, T, 1, half) for t in module.tables(T, d, x.device, x.dtype))
    m = M.reshape(V, N, T, -1)
    mr = m[..., :rotated * d].reshape(V, N, T, rotated, d)
    m1, m2 = mr[..., :half], mr[..., half:]
    rot = torch.cat((m1 * cos + m2 * sin, m2 * cos - m1 * sin), -1).reshape(V, N, T, rotated * d)
    return torch.cat((rot, m[..., rotated * d:]), -1)


def _hip_jac_t_mat_prod(module, M: Tensor, x: Tensor, subsampling=None) -> Optional[Tensor]:
    """The layer rules that have a HIP kernel (csrc/jacobians.hip, csrc/norm_rules.hip, csrc/llama_rules.hip, csrc/attention.hip): activations (ReLU, Sigmoid, Tanh, LeakyReLU,
    LogSigmoid, ELU, SELU, GELU in both forms, SiLU, SoftCap), Flatten / Identity / ActiveIdentity / Dropout(eval), ScaleModule,
    Max/AvgPool1d/2d, Conv1d / Conv2d and ConvTranspose1d / 2d (any groups, zero padding), Pad / ZeroPad2d / Slicing,
    BatchNorm (eval), LayerNorm and GroupNorm (with or without affine parameters; the same visit of the factor serves their
    parameter rules), RMSNorm (likewise), RotaryEmbedding, ScaledDotProductAttention (head dimensions up to 128; the forward output it needs is ``module.output``,
    sub-sampled by ``subsampling`` as ``x`` was), and -- on the same two-dimensional kernels -- Conv3d, ConvTranspose3d, MaxPool3d,
    AvgPool3d.  ``None``: no kernel for this module (custom modules, unsupported options such as ceil_mode) -- the generic autograd
    rule takes over."""
    kind = _activation_kind(module)
    if kind is not None:
        return kernels.act_jac_t(M, x, *kind)
    if isinstance(module, (nn.Flatten, nn.Identity, nn.Dropout, ActiveIdentity)):
        return M.reshape(M.shape[0], *x.shape)
    if isinstance(module, ScaleModule):   # SqrtGGNScaleModule (__init__.py:113-116): the Jacobian is ``weight * I``
        if module.weight == 1.0:
            return M
        Mc = M if M.dim() > 3 else M.unsqueeze(-1)
        return kernels.channel_scale(Mc, M.new_full((Mc.shape[2],), module.weight)).view(M.shape)
    # index modules: the transposed Jacobian of a zero / constant padding is a crop, that of a slicing a scatter into zeros
    # (SqrtGGNPad / SqrtGGNZeroPad2d / SqrtGGNSlicing, __init__.py:110-117) -- no recomputed forward, no autograd
    if isinstance(module, (Pad, nn.ZeroPad2d)):
        pad = tuple(module.padding) if isinstance(module, nn.ZeroPad2d) else tuple(module.pad)
        mode = "constant" if isinstance(module, nn.ZeroPad2d) else module.mode
        if mode == "constant" and len(pad) % 2 == 0 and all(p_ >= 0 for p_ in pad) and len(pad) // 2 <= x.dim():
            g = M
            for i in range(len(pad) // 2):          # F.pad: the last dimension first
                d = g.dim() - 1 - i
                g = g.narrow(d, pad[2 * i], g.shape[d] - pad[2 * i] - pad[2 * i + 1])
            return g.contiguous()
    if isinstance(module, Slicing):
        g = M.new_zeros((M.shape[0],) + tuple(x.shape))
        info = module.slice_info if isinstance(module.slice_info, tuple) else (module.slice_info,)
        g[(slice(None),) + tuple(info)] = M
        return g
    # one-dimensional pooling on the two-dimensional kernels (a row image), as the Conv1d rules do
    if isinstance(module, nn.MaxPool1d) and x.dim() == 3:
        if _single(module.dilation) == 1 and not module.ceil_mode and not module.return_indices:
            ks = _single(module.kernel_size)
            st = _single(module.stride if module.stride is not None else ks)
            g = kernels.maxpool2d_jac_t(M.unsqueeze(3), x.unsqueeze(2), (1, ks), (1, st), (0, _single(module.padding)))
            return g.squeeze(3)
    if isinstance(module, nn.AvgPool1d) and x.dim() == 3:
        if not module.ceil_mode and module.count_include_pad:
            ks = _single(module.kernel_size)
            st = _single(module.stride if module.stride is not None else ks)
            g = kernels.avgpool2d_jac_t(M.unsqueeze(3), (1, x.shape[2]), (1, ks), (1, st), (0, _single(module.padding)))
            return g.squeeze(3)
    if isinstance(module, nn.MaxPool2d) and x.dim() == 4:
        if _pair(module.dilation) == (1, 1) and not module.ceil_mode and not module.return_indices:
            ks = _pair(module.kernel_size)
            return kernels.maxpool2d_jac_t(M, x, ks, _pair(module.stride if module.stride is not None else ks), _pair(module.padding))
    if isinstance(module, nn.AvgPool2d) and x.dim() == 4:
        if not module.ceil_mode and module.count_include_pad and module.divisor_override is None:
            ks = _pair(module.kernel_size)
            return kernels.avgpool2d_jac_t(M, x.shape[2:], ks, _pair(module.stride if module.stride is not None else ks),
                                           _pair(module.padding))
    if isinstance(module, (nn.Conv2d, nn.Conv1d)) and isinstance(module.padding, tuple) and module.padding_mode == "zeros":
        # (a shape neither kernel takes comes back as VIVIT_E_UNSUPPORTED: the caller falls through to the generic rule)
        # a Conv1d is the Conv2d with one row: same kernel; groups > 1: one launch per group on its channel slices
        one_d = isinstance(module, nn.Conv1d)
        W = module.weight.detach()
        if one_d:
            M, W, hw = M.unsqueeze(3), W.unsqueeze(2), (1, x.shape[2])
            st, pd, dl = (1, module.stride[0]), (0, module.padding[0]), (1, module.dilation[0])
        else:
            hw, st, pd, dl = x.shape[2:], module.stride, module.padding, module.dilation
        G = module.groups
        Co = module.out_channels // G
        if G == 1:
            g = kernels.conv2d_jac_t(M, W, hw, st, pd, dl)
        else:
            g = torch.cat([kernels.conv2d_jac_t(M[:, :, i * Co:(i + 1) * Co].contiguous(), W[i * Co:(i + 1) * Co].contiguous(), hw, st, pd, dl)
                           for i in range(G)], 2)
        return g.squeeze(3) if one_d else g
    if (isinstance(module, (nn.ConvTranspose2d, nn.ConvTranspose1d)) and isinstance(module.padding, tuple)
            and getattr(module, "padding_mode", "zeros") == "zeros"):
        g = _hip_convtranspose_jac_t(module, M, x)
        if g is not None:
            return g
    # three-dimensional layers on the two-dimensional kernels (one launch per depth tap / separable pooling)
    if isinstance(module, nn.Conv3d) and x.dim() == 5 and isinstance(module.padding, tuple) and module.padding_mode == "zeros":
        return _hip_conv3d_jac_t(module, M, x)
    if (isinstance(module, nn.ConvTranspose3d) and x.dim() == 5 and isinstance(module.padding, tuple)
            and getattr(module, "padding_mode", "zeros") == "zeros"):
        g = _hip_convtranspose3d_jac_t(module, M, x)
        if g is not None:
            return g
    if isinstance(module, (nn.MaxPool3d, nn.AvgPool3d)) and x.dim() == 5:
        g = _hip_pool3d_jac_t(module, M, x)
        if g is not None:
            return g
    if isinstance(module, _NORMS):
        return _norm_rules(module, M, x, True)[0]
    if isinstance(module, nn.RMSNorm):
        return _rms_norm_rules(module, M, x, True)[0]
    if isinstance(module, RotaryEmbedding):   # the very tables the forward pass used (cached on the module)
        d = module.head_dim(x)
        return kernels.rope_jac_t(M.reshape(M.shape[0], *x.shape), *module.tables(x.shape[1], d, x.device, x.dtype), module.num_heads,
                                  num_kv_heads=module.kv_heads)
    if isinstance(module, ScaledDotProductAttention):
        # (a head dimension above the kernel's 128 has no kernel: the generic rule, before any operand is prepared; sizes beyond
        # the kernel's index arithmetic come back as VIVIT_E_UNSUPPORTED and the caller falls through likewise)
        d = module.head_dim(x)
        lengths = _attention_lengths(module, x, subsampling)
        table = module.bias_for(x.shape[1])
        if d > 128:   # (with lengths the formula in torch: the generic rule's forward pass would not know the sub-sampled ones; with a
            # score modifier likewise: the generic rule would hold [V, N, H, T, T] several times over)
            if lengths is None and module.softcap is None and table is None:
                return None
            return _attention_jac_t_torch(module, M, x, _attention_out(module, x, subsampling), lengths)
        return kernels.attention_jac_t(M.reshape(M.shape[0], *x.shape[:2], -1), x, _attention_out(module, x, subsampling), module.num_heads,
                                       module.scale_for(d), module.causal, num_kv_heads=module.kv_heads, lengths=lengths,
                                       window=module.window, softcap=module.softcap,
                                       bias=None if table is None else table.detach().to(torch.float32).contiguous())
    if isinstance(module, _BATCHNORM) and x.dim() >= 2:
        if _own_params(module):   # the parameter rules want the two row sums of the same pass
            return _bn_eval_rules(module, M, x)[0]
        return kernels.channel_scale(M if M.dim() > 3 else M.unsqueeze(-1), _bn_scale(module)).view(M.shape)
    return None


def _convtranspose2d_input(M: Tensor, W: Tensor, ks, st, pd, dl, G: int, hq) -> Optional[Tensor]:
    """``g[ci, q] = sum_{co, k} W[ci, co, k] M[co, q s - p + k d]`` for ``M [V, N, Cout, H', W']``, ``W [Cin, Cout / G, kh,
    kw]`` -> ``[V, N, Cin, *hq]`` on the HIP kernel of the convolution's input rule.

    With the kernel index reversed (k' = K - 1 - k) this is the stride-1 input rule
    ``sum_{o, k'} W'[o, ci, k'] M[o, y + p' - k' d]`` of a convolution with weight ``W'[co, ci, k'] = W[ci, co, K - 1 - k']``
    and padding ``p' = (K - 1) d - p``, evaluated at ``y = q s`` -- the kernel computes every y and the stride picks every
    s-th (s^2 of the work is discarded for s > 1; transposed convolutions are rare on this path).  ``None`` when p' would be
    negative or the kernel's channel limit is exceeded."""
    pad2 = tuple((k - 1) * d - p for k, d, p in zip(ks, dl, pd))
    Cin = W.shape[0]
    Co, Ci = W.shape[1], Cin // G
    if min(pad2) < 0 or Co * ks[0] * ks[1] > 1024:
        return None
    # input size of the stride-1 rule whose output size is M's:  H' = full + 2 p' - d (K - 1)  <=>  full = H' + 2 p - d (K - 1)
    full = tuple(h + 2 * p - d * (k - 1) for h, p, d, k in zip(M.shape[3:], pd, dl, ks))
    if any(f < (q - 1) * s_ + 1 for f, q, s_ in zip(full, hq, st)):
        return None
    parts = []
    for g in range(G):
        Wg = W[g * Ci:(g + 1) * Ci].transpose(0, 1).flip(2, 3).contiguous()            # [Co, Ci, kh, kw], reversed taps
        Mg = M if G == 1 else M[:, :, g * Co:(g + 1) * Co].contiguous()
        parts.append(kernels.conv2d_jac_t(Mg, Wg, full, (1, 1), pad2, dl))
    out = parts[0] if G == 1 else torch.cat(parts, 2)
    return out[..., ::st[0], ::st[1]][..., :hq[0], :hq[1]].contiguous()


def _hip_convtranspose_jac_t(module, M: Tensor, x: Tensor) -> Optional[Tensor]:
    """Input rule of ConvTranspose1d/2d (convtransposend.py:9-30): the transposed Jacobian of y = conv_transpose(x, W) is a
    forward convolution of ``M`` with ``W`` (:func:`_convtranspose2d_input`); a 1-D layer is the 2-D one with a single row."""
    one_d = isinstance(module, nn.ConvTranspose1d)
    W = module.weight.detach()
    if one_d:
        M, W = M.unsqueeze(3), W.unsqueeze(2)
        ks, st, pd, dl = (1, module.kernel_size[0]), (1, module.stride[0]), (0, module.padding[0]), (1, module.dilation[0])
        hq = (1, x.shape[2])
    else:
        ks, st, pd, dl = module.kernel_size, module.stride, module.padding, module.dilation
        hq = tuple(x.shape[2:])
    out = _convtranspose2d_input(M, W, ks, st, pd, dl, module.groups, hq)
    if out is None:
        return None
    return out.squeeze(3) if one_d else out


def _generic_jac_t_mat_prod(module, M: Tensor, x: Tensor) -> Tensor:
    """The generic rule of :func:`_jac_t_mat_prod` for a module without a kernel: batched vector-Jacobian product through a recomputed
    forward (bypasses hooks)."""
    with torch.enable_grad():
        xi = x.detach().requires_grad_(True)
        y = module.forward(xi)
        (g,) = torch.autograd.grad(y, xi, grad_outputs=M.reshape(M.shape[0], *y.shape), is_grads_batched=True)
    return g


def _jac_t_mat_prod(module, M: Tensor, x: Tensor, subsampling=None) -> Tensor:
    """Apply the transposed input-Jacobian of ``module`` to ``M`` [V, N, *out] -> [V, N, *in].  ``subsampling``: the indices ``x`` was
    sub-sampled with (rules that read ``module.output`` sub-sample it likewise)."""
    if isinstance(module, nn.Linear):   # (any number of extra dimensions between batch and features: linear.py:38-39)
        if M.is_cuda and M.dtype == torch.float32:
            O = M.shape[-1]
            return kernels.gemm_nn(M.reshape(-1, O), module.weight.detach()).view(*M.shape[:-1], -1)
        return M @ module.weight.detach()
    if isinstance(module, Permute):     # a view on every device: the inverse permutation behind the leading V axis (no copy, no kernel)
        return M.permute((0,) + tuple(d + 1 for d in module.inverse_dims()))
    if isinstance(module, nn.Dropout) and module.training and module.p > 0:
        raise NotImplementedError("Dropout must be in eval mode")
    if isinstance(module, _BATCHNORM) and module.training:
        raise NotImplementedError("BatchNorm must be in eval mode")
    if M.is_cuda and M.dtype == torch.float32:
        try:
            g = _hip_jac_t_mat_prod(module, M, x, subsampling)
        except _lib.VivitHipError as exc:  # a shape beyond a kernel's launch limits: the generic rule below
            if exc.status != _lib.VIVIT_E_UNSUPPORTED:
                raise
            g = None
        if g is not None:
            return g
    elif isinstance(module, ScaledDotProductAttention):   # non-HIP or non-fp32 tensors: the same formula in torch
        return _attention_jac_t_torch(module, M, x, _attention_out(module, x, subsampling), _attention_lengths(module, x, subsampling))
    # non-HIP or non-fp32 tensors (or a size beyond the kernels' index arithmetic): the same formulas in torch, never autograd
    if isinstance(module, nn.RMSNorm):
        return _rms_norm_jac_t_torch(module, M, x)
    if isinstance(module, RotaryEmbedding):
        return _rope_jac_t_torch(module, M, x)
    return _generic_jac_t_mat_prod(module, M, x)


# ---------------------------------------------------------------------------------------------
class BatchGrad(_Extension):
    """Per-sample gradients of the mini-batch loss (BackPACK ``BatchGrad``)."""

    savefield = "grad_batch"
    uses_grad = True   # reads autograd's gradient: the extensions' stream waits for the backward pass at every hook (engine.py)

    def __init__(self, subsampling: Optional[List[int]] = None, factorised: bool = False):
        super().__init__(subsampling)
        self._factorised = factorised

    def apply(self, ctx, module, g_out):
        params = _own_params(module)
        if not params or isinstance(module, _LOSSES):
            return
        sub = self.get_subsampling()
        g = subsample(g_out.detach(), 0, sub).unsqueeze(0)  # [1, N, *out]
        x = subsample(module.input0.detach(), 0, sub)
        for name, p in params:
            if self._factorised and isinstance(module, nn.Linear) and name == "weight" and g.dim() == 3:
                setattr(p, self.savefield, LinearFactor(g[0], x))
            else:
                setattr(p, self.savefield, _param_factor_of(module, name, g, x, sub)[0])


# ---------------------------------------------------------------------------------------------
def _ce_position_weights(module, target: Tensor, C: int) -> Tensor:
    """``omega [N, *D]`` (fp64): the loss Hessian of ``nn.CrossEntropyLoss`` w.r.t. the logits of position ``i = (n, l)`` is
    ``omega_i (diag p_i - p_i p_i^T)``.  With ``w`` the class weights (ones if absent), ``wbar = mean_c w_c``, ``eps`` the label smoothing:

    * class-index targets ``y [N, *D]``: position ``i`` counts iff ``y_i != ignore_index`` and ``0 <= y_i < C``; then
      ``a_i = (1 - eps) w[y_i] + eps wbar``, else ``a_i = 0``; ``omega_i = a_i / norm`` with ``norm`` the sum of ``w[y_i]`` over the
      counted positions of the whole batch ('mean') or 1 ('sum');
    * probability targets ``t [N, C, *D]`` (floating point): ``omega_i = sum_c w_c ((1 - eps) t_ic + eps / C) / norm``, ``norm`` the
      number of positions ``N L`` ('mean') or 1; there is no ``ignore_index``.

    ``a_i == 0`` gives ``omega_i = 0`` even when ``norm == 0`` (every target ignored: torch's loss is NaN, the factor is zero); a
    negative ``omega_i`` (negative class weights) becomes NaN under the square root; a target outside ``[0, C)`` that is not
    ``ignore_index`` has weight 0 and indexes nothing.  Torch ops only, nothing comes back to the host."""
    eps = float(module.label_smoothing)
    w = None if module.weight is None else module.weight.detach().to(target.device, torch.float64)
    mean = module.reduction == "mean"
    if target.is_floating_point():
        mix = (1.0 - eps) * target.detach().to(torch.float64) + eps / C
        if w is not None:
            mix = mix * w.view(1, C, *([1] * (mix.dim() - 2)))
        a = mix.sum(dim=1)
        return a / a.numel() if mean else a
    y = target.detach()
    counted = (y != module.ignore_index) & (y >= 0) & (y < C)
    if w is None:
        wy = counted.to(torch.float64)
        a = wy                                                             # (1 - eps) + eps, exactly
    else:
        wy = torch.where(counted, w[torch.where(counted, y, torch.zeros_like(y))], torch.zeros((), dtype=torch.float64, device=y.device))
        a = wy if eps == 0.0 else torch.where(counted, (1.0 - eps) * wy + eps * w.mean(), torch.zeros_like(wy))
    if not mean:
        return a
    return torch.where(a == 0, torch.zeros_like(a), a / wy.sum())


def _ce_position_scale(module, out: Tensor, mult: int) -> Optional[Tensor]:
    """``s [N, *D] = sqrt(omega / mult)`` in the dtype of ``out`` (:func:`_ce_position_weights`; ``mult = M`` for the sampled factor),
    or None for a loss that recorded no target (nothing to look at: the unweighted factor).  Class-index targets of HIP fp32 logits:
    one kernel pair on the device (``kernels.ce_target_scales``), which for a default loss with nothing ignored gives the very float
    ``1 / sqrt(mult norm)`` of the unweighted path; otherwise torch ops.  Never a host synchronisation: the factor pass runs on its
    own stream beside the backward pass (engine.py)."""
    target = getattr(module, "input1", None)
    if not isinstance(target, Tensor):
        return None
    C = out.shape[1]
    if not target.is_floating_point() and out.is_cuda and out.dtype == torch.float32 and target.device == out.device:
        w = None if module.weight is None else module.weight.detach().to(out.device, torch.float32)
        return kernels.ce_target_scales(target.detach().long(), C, weight=w, ignore_index=module.ignore_index,
                                        label_smoothing=module.label_smoothing, mean=module.reduction == "mean", mult=mult)
    return (_ce_position_weights(module, target.to(out.device), C) / mult).sqrt().to(out.dtype)


def _scaled_positions(S: Tensor, s: Tensor) -> Tensor:
    """``S [V, N, C, *D]`` times the scale ``s [N, *D]`` of its positions; zeros where ``s == 0`` whatever ``S`` holds there (a padded
    position's logits may be NaN, and ``0 * NaN`` must not reach the factor)."""
    s = s.unsqueeze(0).unsqueeze(2)
    return torch.where(s == 0, torch.zeros((), dtype=S.dtype, device=S.device), S * s)


def _loss_hessian_sqrt_positions(module, out: Tensor, strategy: str, mc_samples: int, samples: Optional[Tensor]) -> Tensor:
    """Symmetric factor S [V, N, C, *D] of the loss Hessian w.r.t. an output with positions, ``out [N, C, *D]``, ``L = prod(D)``.

    CrossEntropyLoss (a softmax over the classes at every position; the Hessian at position ``i`` is ``omega_i (diag p_i - p_i p_i^T)``
    with ``omega`` of :func:`_ce_position_weights` -- ``ignore_index``, class ``weight``, ``label_smoothing`` and probability targets
    included; ``1 / (N L)`` for a default 'mean' loss with nothing ignored): exact, ``V = C L``, row ``v = c' L + l'``,
    ``S[v, n, c, l] = [l = l'] sqrt(p[n, c', l]) ([c = c'] - p[n, c, l]) sqrt(omega[n, l])``; sampled, ``V = M``,
    ``S[m, n, c, l] = (p[n, c, l] - [c = idx[m, n, l]]) sqrt(omega[n, l] / M)`` with class indices ``idx [M, N, *D]`` -- ``samples`` of an
    integer dtype, the argmax of one-hot ``samples [M, N, C, *D]``, or drawn here from ``p``.  A position with ``omega = 0`` is exact
    zeros.  HIP fp32 tensors: one kernel (``kernels.ce_sqrt_hessian_positions_w``, in the memory format of ``out``); otherwise the same
    formulas in torch, no autograd.  A loss that recorded no target: ``omega = 1 / norm``, ``norm = N L`` for 'mean'
    (``kernels.ce_sqrt_hessian_positions``).
    MSELoss ('mean' averages over ``N C L`` elements): ``sqrt(2 / norm) I`` as ``[C L, N, C, *D]``, or ``M`` normal samples."""
    N, C, D = out.shape[0], out.shape[1], tuple(out.shape[2:])
    L = math.prod(D)
    red = module.reduction
    if red not in ("mean", "sum"):
        raise NotImplementedError(f"reduction={red}")
    if isinstance(module, nn.CrossEntropyLoss):
        norm = N * L if red == "mean" else 1
        hip = out.is_cuda and out.dtype == torch.float32
        if strategy == "exact":
            s = _ce_position_scale(module, out, 1)
            if hip:
                if s is not None:
                    return kernels.ce_sqrt_hessian_positions_w(out, s)
                return kernels.ce_sqrt_hessian_positions(out, 1.0 / math.sqrt(norm))
            p = out.softmax(dim=1).reshape(N, C, L)
            eye_c = torch.eye(C, dtype=out.dtype, device=out.device)
            eye_l = torch.eye(L, dtype=out.dtype, device=out.device)
            inner = p.sqrt().permute(1, 0, 2).unsqueeze(2) * (eye_c[:, None, :, None] - p.unsqueeze(0))      # [c', n, c, l]
            S = inner.unsqueeze(1) * eye_l[None, :, None, None, :]                                           # [c', l', n, c, l]
            S = S.reshape(C * L, N, C, *D)
            return _scaled_positions(S, s) if s is not None else S / math.sqrt(norm)
        if samples is None:
            p = out.softmax(dim=1)
            idx = torch.multinomial(p.movedim(1, -1).reshape(N * L, C), mc_samples, replacement=True).t().reshape(mc_samples, N, *D)
        elif samples.is_floating_point():
            if tuple(samples.shape[1:]) != tuple(out.shape):
                raise ValueError(f"one-hot samples must be [M, {', '.join(map(str, out.shape))}], got {tuple(samples.shape)}")
            idx = samples.argmax(dim=2)
        else:
            if tuple(samples.shape[1:]) != (N,) + D:
                raise ValueError(f"class-index samples must be [M, {', '.join(map(str, (N,) + D))}], got {tuple(samples.shape)}")
            idx = samples
        s = _ce_position_scale(module, out, idx.shape[0])
        scale = 1.0 / math.sqrt(idx.shape[0] * norm)
        if hip:
            if s is not None:
                return kernels.ce_sqrt_hessian_positions_w(out, s, idx=idx.to(out.device, torch.int32))
            return kernels.ce_sqrt_hessian_positions(out, scale, idx=idx.to(out.device, torch.int32))
        onehot = F.one_hot(idx.to(out.device, torch.long), C).movedim(-1, 2).to(out.dtype)                   # [M, N, C, *D]
        S = out.softmax(dim=1).unsqueeze(0) - onehot
        return _scaled_positions(S, s) if s is not None else S * scale
    if isinstance(module, nn.MSELoss):
        norm = N * C * L if red == "mean" else 1
        if strategy == "exact":
            S = torch.eye(C * L, dtype=out.dtype, device=out.device).unsqueeze(1).expand(C * L, N, C * L)
            return (S * math.sqrt(2.0 / norm)).view(C * L, N, C, *D)
        if samples is None:
            samples = torch.randn(mc_samples, N, C, *D, dtype=out.dtype, device=out.device)
        elif tuple(samples.shape[1:]) != tuple(out.shape):
            raise ValueError(f"samples must be [M, {', '.join(map(str, out.shape))}], got {tuple(samples.shape)}")
        return samples.to(out.device, out.dtype) * math.sqrt(2.0 / (samples.shape[0] * norm))
    raise NotImplementedError(type(module).__name__)


def _loss_hessian_sqrt(module, strategy: str, mc_samples: int, samples: Optional[Tensor]) -> Tensor:
    """Symmetric factor S [V, N, C] of the loss Hessian w.r.t. the model output ``[N, C]``; ``[V, N, C, *D]`` for an output with
    positions ``[N, C, *D]`` (:func:`_loss_hessian_sqrt_positions`).  CrossEntropyLoss on ``[N, C]`` is the case of one position per
    sample: the factor of sample ``n`` times ``sqrt(omega_n)`` (``sqrt(omega_n / M)`` sampled) with ``omega`` of
    :func:`_ce_position_weights`, exact zeros where ``omega_n = 0``."""
    out = module.input0.detach()
    if out.dim() > 2:
        return _loss_hessian_sqrt_positions(module, out, strategy, mc_samples, samples)
    if out.dim() != 2:
        raise NotImplementedError("loss input must be [N, C] or [N, C, *D]")
    N, C = out.shape
    red = module.reduction
    if red not in ("mean", "sum"):
        raise NotImplementedError(f"reduction={red}")
    if isinstance(module, nn.CrossEntropyLoss) and out.is_cuda and out.dtype == torch.float32 and C * 4 <= 60 * 1024:
        norm = N if red == "mean" else 1
        if strategy == "exact":
            s = _ce_position_scale(module, out, 1)
            if s is not None:
                return kernels.ce_sqrt_hessian_w(out, s)
            return kernels.ce_sqrt_hessian(out, 1.0 / math.sqrt(norm))     # softmax + sqrt(p_v)(delta_vc - p_c) in one kernel
        if samples is None:
            idx = torch.multinomial(out.softmax(dim=1), mc_samples, replacement=True)  # [N, M]
            samples = F.one_hot(idx.t(), C).to(out.dtype)  # [M, N, C]
        samples = samples.to(out.device, out.dtype)
        s = _ce_position_scale(module, out, samples.shape[0])
        if s is not None:
            return kernels.ce_sqrt_hessian_w(out, s, onehot=samples)
        return kernels.ce_sqrt_hessian(out, 1.0 / math.sqrt(samples.shape[0] * norm), onehot=samples)
    if isinstance(module, nn.CrossEntropyLoss):
        p = out.softmax(dim=1)
        norm = N if red == "mean" else 1
        if strategy == "exact":
            sq = p.sqrt()
            # H_n = diag(p_n) - p_n p_n^T = sum_v S[v,n,:] S[v,n,:]^T,  S[v,n,c] = sqrt(p_nv)(delta_vc - p_nc)
            S = torch.einsum("nv,vc->vnc", sq, torch.eye(C, dtype=out.dtype, device=out.device)) - torch.einsum(
                "nv,nc->vnc", sq, p
            )
            s = _ce_position_scale(module, out, 1)
            return _scaled_positions(S, s) if s is not None else S / math.sqrt(norm)
        if samples is None:
            idx = torch.multinomial(p, mc_samples, replacement=True)  # [N, M]
            samples = F.one_hot(idx.t(), C).to(out.dtype)  # [M, N, C]
        S = p.unsqueeze(0) - samples.to(out.device, out.dtype)
        s = _ce_position_scale(module, out, samples.shape[0])
        return _scaled_positions(S, s) if s is not None else S / math.sqrt(samples.shape[0] * norm)
    if isinstance(module, nn.MSELoss):
        norm = N * C if red == "mean" else 1
        if strategy == "exact":
            S = torch.eye(C, dtype=out.dtype, device=out.device).unsqueeze(1).expand(C, N, C)
            return S * math.sqrt(2.0 / norm)
        if samples is None:
            samples = torch.randn(mc_samples, N, C, dtype=out.dtype, device=out.device)
        return samples.to(out.device, out.dtype) * math.sqrt(2.0 / (samples.shape[0] * norm))
    raise NotImplementedError(type(module).__name__)


class _SqrtGGN(_Extension):
    strategy = "exact"
    uses_grad = False   # reads forward activations and the back-propagated factor only, never ``g_out``

    def __init__(self, subsampling=None, mc_samples: int = 1, samples: Optional[Tensor] = None, factorised: bool = False):
        super().__init__(subsampling)
        self._mc_samples = mc_samples
        self._samples = samples  # externally supplied MC one-hots [M, N, C] (parity needs them)
        self._factorised = factorised

    def get_num_mc_samples(self) -> int:
        return self._mc_samples

    def _store(self, module, name, param, M, x, subsampling=None):
        if self._factorised and isinstance(module, nn.Linear) and name == "weight" and M.dim() == 3:
            setattr(param, self.savefield, LinearFactor(M, x))
        else:
            setattr(param, self.savefield, _param_factor_of(module, name, M, x, subsampling))

    def apply(self, ctx, module, g_out):
        sub = self.get_subsampling()
        if isinstance(module, _LOSSES):
            S = _loss_hessian_sqrt(module, self.strategy, self._mc_samples, self._samples)
            ctx.put(self, module.input0, subsample(S, 1, sub))
            return
        M = ctx.pop(self, module.output)
        if M is None:
            return
        if isinstance(module, SumModule):  # identity Jacobian w.r.t. every summand (SqrtGGNSumModule)
            for inp in module.inputs:
                if inp.requires_grad:
                    ctx.put(self, inp, M)
            return
        if isinstance(module, ProductModule):  # y = a * b: M * b goes to a, M * a to b (the same tensor twice: both, added)
            a, b = (subsample(t.detach(), 0, sub) for t in module.inputs)
            need = tuple(t.requires_grad for t in module.inputs)
            if any(need):
                if M.is_cuda and M.dtype == torch.float32:
                    parts = kernels.gate_jac_t(M.reshape(M.shape[0], *a.shape), a, b, want=need)
                else:
                    parts = (M * b.unsqueeze(0) if need[0] else None, M * a.unsqueeze(0) if need[1] else None)
                for inp, g in zip(module.inputs, parts):
                    if g is not None:
                        ctx.put(self, inp, g)
            return
        if isinstance(module, ScaledDotProductCrossAttention):  # dQ goes to the queries, dK | dV to the second sequence
            need = tuple(t.requires_grad for t in module.inputs)
            if any(need):   # (a frozen memory: the key owner is not launched)
                for inp, g in zip(module.inputs, _cross_attention_jac_t(module, M, sub, need)):
                    if g is not None:
                        ctx.put(self, inp, g)
            return
        x = subsample(module.input0.detach(), 0, sub)
        for name, p in _own_params(module):
            self._store(module, name, p, M, x, subsampling=sub)
        if module.input0.requires_grad:
            ctx.put(self, module.input0, _jac_t_mat_prod(module, M, x, sub))


class SqrtGGNExact(_SqrtGGN):
    """Materialised ``V_t`` with the exact loss Hessian (BackPACK ``SqrtGGNExact``)."""

    savefield = "sqrt_ggn_exact"
    strategy = "exact"

    def __init__(self, subsampling=None, factorised: bool = False):
        super().__init__(subsampling, factorised=factorised)


class SqrtGGNMC(_SqrtGGN):
    """Materialised ``V_t`` with an MC-sampled loss Hessian (BackPACK ``SqrtGGNMC``)."""

    savefield = "sqrt_ggn_mc"
    strategy = "sampling"

    def __init__(self, mc_samples: int = 1, subsampling=None, samples: Optional[Tensor] = None, factorised: bool = False):
        super().__init__(subsampling, mc_samples, samples, factorised=factorised)


# ---------------------------------------------------------------------------------------------
def _materialised_closures(V_t: Tensor):
    """Closures over a materialised ``V_t`` (vivit/extensions/secondorder/vivit/base.py:96-130)."""

    def gram_mat(out=None, beta=0.0):
        return pairwise_dot(V_t, start_dim=2, flatten=False, out=out, beta=beta)

    def dp_add(acc):  # data parallel: this rank's rows of V_t into a vivit_amd.distributed.BatchShardedGram
        if V_t[0, 0].numel() < DP_ROWS_MAX_COLUMNS:
            acc.add_factor_rows(V_t)
        else:
            acc.add_factor(V_t)

    return {
        "V_mat_prod": lambda mat: Vmp(V_t, mat, 2),
        "V_t_mat_prod": lambda mat: mVp(V_t, mat, 2),
        "gram_mat": gram_mat,
        "dp_add": dp_add,
        # explicit factor [C, N, *param] and its leading shape: used when the parameter side of a group is the
        # smaller one (vivit_amd.linalg.utils.parameter_side_symeig)
        "factor": lambda: V_t,
        "shape_cn": tuple(V_t.shape[:2]),
    }


def _linear_weight_closures(s: Tensor, z: Tensor):
    """Factorised closures for a Linear weight: ``V_t[c,n,o,i] = s[c,n,o] z[n,i]`` never exists.

    vivit/extensions/secondorder/vivit/linear.py:44-75.  Gram: two small SYRKs plus the fused
    Hadamard kernel (K1'); products: one tall GEMM with ``z`` plus a length-C contraction.
    """
    C, N, O = s.shape
    s = s.contiguous()
    z = z.contiguous()

    def gram_mat(out=None, beta=0.0):
        Gz = kernels.gram_syrk(z)                      # [N, N]
        Gs = kernels.gram_syrk(s.reshape(C * N, O))    # [CN, CN]
        out2d = None if out is None else out.view(C * N, C * N)
        G = kernels.gram_hadamard(Gz, Gs, C, N, out=out2d, alpha=1.0, beta=beta)
        return G.view(C, N, C, N)

    def V_mat_prod(mat):  # [F, C, N] -> [F, O, I]     "cno,vcn,ni->voi"
        Fdim = mat.shape[0]
        T = kernels.class_contract(mat, s).view(Fdim * O, N)
        return kernels.gemm_nn(T, z).view(Fdim, O, z.shape[1])

    def V_t_mat_prod(mat):  # [F, O, I] -> [F, C, N]   "cno,voi,ni->vcn"
        Fdim = mat.shape[0]
        U = kernels.gemm_nt(mat.reshape(Fdim * O, -1), z).view(Fdim, O, N)
        return kernels.class_expand(s, U)

    def factor():  # the explicit V_t[c,n,o,i] = s[c,n,o] z[n,i]; only asked for when O*I is small
        return LinearFactor(s, z).materialise()

    return {"V_mat_prod": V_mat_prod, "V_t_mat_prod": V_t_mat_prod, "gram_mat": gram_mat, "factor": factor,
            "shape_cn": (C, N), "dp_add": lambda acc: acc.add_linear(s, z)}


def _seq_linear_plan(C: int, N: int, T: int, O: int, I: int, workspace_bytes: Optional[int] = None, kappa: Optional[float] = None,
                     syrk_workspace=None):
    """How ``_linear_seq_weight_closures`` builds its Gram matrix; pure arithmetic on the sizes (no tensor, no device).

    Multiply-adds, symmetric halves: route A (expanded) ``(C N T)^2 / 2 * O + (N T)^2 / 2 * I``, route B (explicit, chunked)
    ``(C N)^2 / 2 * O I + C N T O I``.  Route A is taken when ``kappa * macs_A <= macs_B`` and one row of T x T blocks fits the
    workspace.  Returns ``{"route", "macs_A", "macs_B", "slabs", "chunks"}``:

    * ``slabs`` (route A): ``(r0, r1, cols)``: ranges ``r0 .. r1 - 1`` of the rows ``(c, n) = c N + n`` of G, in order, covering
      ``0 .. C N``, and the number of columns ``0 .. cols - 1`` the slab computes: ``cols = r1``, its own last row (lower block
      trapezoid).  A slab is a range of whole classes or a range of samples of one class, so its rows of ``s'`` are contiguous;
      its block of Gs, ``[(r1 - r0) T, cols T]`` floats, fits HALF the workspace.
    * ``chunks`` (route B): ``(o0, o1)`` ranges of the output features, a chunk ``[C, N, o1 - o0, I]`` of the factor and the scratch
      buffer of its SYRK together within the workspace (one feature at least).

    The scratch buffer of the GEMM / SYRK launchers holds the bf16 pieces of large operands, 1.5 times their size.  Route A keeps it
    in the other half of the workspace by cutting its products into pieces (``_gemm_nt_within``); route B shrinks the chunk until
    both fit.  ``syrk_workspace(n, p)`` (default ``kernels.gram_syrk_workspace_bytes``, a host-side query) gives those bytes."""
    W = (SEQ_LINEAR_WORKSPACE_BYTES if workspace_bytes is None else workspace_bytes) // 2
    kappa = SEQ_LINEAR_KAPPA if kappa is None else kappa
    syrk_workspace = kernels.gram_syrk_workspace_bytes if syrk_workspace is None else syrk_workspace
    n = C * N
    macs_A = (n * T) ** 2 / 2 * O + (N * T) ** 2 / 2 * I
    macs_B = n ** 2 / 2 * O * I + n * T * O * I
    plan = {"macs_A": macs_A, "macs_B": macs_B, "slabs": [], "chunks": []}
    fits = 4 * T * n * T <= W                      # the last row's blocks: the widest a one-row slab gets
    if fits and kappa * macs_A <= macs_B:
        plan["route"] = "A"
        r0 = 0
        while r0 < n:
            # the largest r1 with 4 (r1 - r0) T * r1 T <= W
            r1 = min(n, int((r0 + math.sqrt(r0 * r0 + W / (T * T))) / 2))
            while r1 < n and 4 * (r1 + 1 - r0) * T * (r1 + 1) * T <= W:
                r1 += 1
            while 4 * (r1 - r0) * T * r1 * T > W:
                r1 -= 1
            c0, n0 = divmod(r0, N)
            if n0 == 0 and r1 - r0 >= N:
                r1 = r0 + (r1 - r0) // N * N       # whole classes
            else:
                r1 = min(r1, (c0 + 1) * N)         # samples of class c0
            plan["slabs"].append((r0, r1, r1))
            r0 = r1
    else:
        plan["route"] = "B"
        step = max(1, min(O, 2 * W // (4 * n * I)))
        while step > 1 and 4 * n * step * I + syrk_workspace(n, step * I) > 2 * W:
            step = step * 7 // 8
        plan["chunks"] = [(o0, min(O, o0 + step)) for o0 in range(0, O, step)]
    return plan


def _gemm_nt_within(A: Tensor, B: Tensor, cap: int, out: Optional[Tensor] = None) -> Tensor:
    """``A B^T`` by ``kernels.gemm_nt`` on pieces of the rows of ``A`` and ``B`` small enough for the launcher's scratch buffer to
    stay within ``cap`` bytes (pieces of ``GEMM_PIECE_MIN_ROWS`` rows at the least); into ``out`` (a row-strided view) if given."""
    m, k = A.shape
    nb = B.shape[0]
    mp, bp = m, nb
    while kernels.gemm_workspace_bytes(mp, bp, k) > cap and max(mp, bp) > GEMM_PIECE_MIN_ROWS:
        if mp >= bp:
            mp = (mp + 1) // 2
        else:
            bp = (bp + 1) // 2
    if out is None:
        out = torch.empty((m, nb), dtype=A.dtype, device=A.device)
    for i in range(0, m, mp):
        for j in range(0, nb, bp):
            kernels.gemm_nt(A[i:i + mp], B[j:j + bp], out=out[i:i + mp, j:j + bp])
    return out


def _gram_within(A: Tensor, cap: int, out: Optional[Tensor] = None) -> Tensor:
    """``A A^T``: the SYRK where its scratch buffer stays within ``cap`` bytes, ``_gemm_nt_within`` otherwise; into ``out`` (a
    row-strided view) if given."""
    if kernels.gram_syrk_workspace_bytes(A.shape[0], A.shape[1]) <= cap:
        return kernels.gram_syrk(A, out=out)
    return _gemm_nt_within(A, A, cap, out=out)


def _slab_of_gs(s2: Tensor, r0: int, r1: int, cols: int, T: int, cap: int) -> Tensor:
    """Rows ``r0 T .. r1 T - 1``, columns ``0 .. cols T - 1`` of ``Gs = s' s'^T``: the columns left of the slab's diagonal block by
    GEMM, the diagonal block itself (where the slab ends with it, ``cols = r1``) by the SYRK, which computes half of it."""
    if (r0, cols) == (0, r1):
        return _gram_within(s2[:r1 * T], cap)
    rows = s2[r0 * T:r1 * T]
    Gs = torch.empty(((r1 - r0) * T, cols * T), dtype=s2.dtype, device=s2.device)
    if r0 > 0:
        _gemm_nt_within(rows, s2[:r0 * T], cap, out=Gs[:, :r0 * T])
    if cols == r1:
        _gram_within(rows, cap, out=Gs[:, r0 * T:])
    else:
        _gemm_nt_within(rows, s2[r0 * T:cols * T], cap, out=Gs[:, r0 * T:])
    return Gs


def _linear_seq_weight_closures(s: Tensor, z: Tensor):
    """Factorised closures for a Linear weight on a sequence input: ``s [C, N, *A, O]`` the factor at the module output, ``z [N, *A, I]``
    the input, ``T = prod(A)``.  ``V_t[c,n,o,i] = sum_t s[c,n,t,o] z[n,t,i]`` ([C, N, O, I]) exists only when ``factor()`` or ``dp_add``
    ask for it (HIP fp32 tensors).

    Gram, by :func:`_seq_linear_plan`: route A, ``G[(c,n),(e,m)] = sum_{t,u} Gs[(c,n,t),(e,m,u)] Gz[(n,t),(m,u)]`` with the Gram
    matrices ``Gs`` of ``s' = [C N T, O]`` (in row slabs within ``SEQ_LINEAR_WORKSPACE_BYTES``) and ``Gz`` of ``z' = [N T, I]``, summed
    by ``kernels.gram_seq_reduce``, lower block trapezoid, then mirrored; or route B, the explicit factor in chunks of the output
    features, each added by the SYRK.  Products: the chains of :func:`_linear_weight_closures` on ``s'``, ``z'`` with ``N T`` for ``N``.
    """
    C, N, O = s.shape[0], s.shape[1], s.shape[-1]
    I = z.shape[-1]
    s3 = s.reshape(C, N, -1, O).contiguous()       # [C, N, T, O]
    T = s3.shape[2]
    s2 = s3.view(C * N * T, O)                     # s'
    z2 = z.reshape(N * T, I).contiguous()          # z'
    n = C * N

    def gram_A(G, beta, slabs):
        cap = SEQ_LINEAR_WORKSPACE_BYTES // 2
        Gz = _gram_within(z2, cap)                                             # [N T, N T]
        for r0, r1, cols in slabs:                 # rows r0 .. r1 - 1 against the columns 0 .. cols - 1
            Gs = _slab_of_gs(s2, r0, r1, cols, T, cap)                         # [(r1 - r0) T, cols T]
            c0, n0 = divmod(r0, N)
            if n0 == 0 and (r1 - r0) % N == 0:     # whole classes c0 .. c1 - 1 against the classes 0 .. cols / N - 1
                kernels.gram_seq_reduce(Gz, Gs, (r1 - r0) // N, N, cols // N, N, T, out=G[r0:r1, :cols], alpha=1.0, beta=beta)
            else:                                  # samples n0 .. n1 - 1 of class c0: the classes below it, then its own samples 0 .. mc - 1
                n1, mc = r1 - c0 * N, cols - c0 * N
                if c0 > 0:
                    kernels.gram_seq_reduce(Gz[n0 * T:n1 * T], Gs[:, :c0 * N * T], 1, n1 - n0, c0, N, T, out=G[r0:r1, :c0 * N],
                                            alpha=1.0, beta=beta)
                kernels.gram_seq_reduce(Gz[n0 * T:n1 * T, :mc * T], Gs[:, c0 * N * T:], 1, n1 - n0, 1, mc, T,
                                        out=G[r0:r1, c0 * N:cols], alpha=1.0, beta=beta)
            del Gs
        return kernels.symmetrize_lower(G)         # the T x T sums of (i, j) and (j, i) differ in their order: one is kept

    def gram_B(G, beta, chunks):
        xa = z2.view(N, T, I).transpose(1, 2).unsqueeze(2).contiguous()        # [N, I, 1, T]: a 1 x 1 convolution over the T positions
        for o0, o1 in chunks:
            Mc = s3[..., o0:o1].transpose(2, 3).unsqueeze(3).contiguous()      # [C, N, o1 - o0, 1, T]
            Vc = kernels.conv2d_weight_mjp(Mc, xa, (1, 1), (1, 1), (0, 0), (1, 1))
            kernels.gram_syrk(Vc.reshape(n, -1), out=G, alpha=1.0, beta=beta)
            del Vc
            beta = 1.0
        return G

    def gram_mat(out=None, beta=0.0):
        plan = _seq_linear_plan(C, N, T, O, I)
        G = torch.empty((n, n), dtype=torch.float32, device=s.device) if out is None else out.view(n, n)
        if out is None:
            beta = 0.0
        G = gram_A(G, beta, plan["slabs"]) if plan["route"] == "A" else gram_B(G, beta, plan["chunks"])
        return G.view(C, N, C, N)

    def V_mat_prod(mat):  # [F, C, N] -> [F, O, I]     "cnto,vcn,nti->voi"
        Fdim = mat.shape[0]
        rep = mat.unsqueeze(-1).expand(Fdim, C, N, T).reshape(Fdim, C, N * T)
        U = kernels.class_contract(rep, s2.view(C, N * T, O)).view(Fdim * O, N * T)
        return kernels.gemm_nn(U, z2).view(Fdim, O, I)

    def V_t_mat_prod(mat):  # [F, O, I] -> [F, C, N]   "cnto,voi,nti->vcn"
        Fdim = mat.shape[0]
        U = kernels.gemm_nt(mat.reshape(Fdim * O, I), z2).view(Fdim, O, N * T)
        return kernels.class_expand(s2.view(C, N * T, O), U).view(Fdim, C, N, T).sum(3)

    def factor():  # the explicit V_t; only asked for by the parameter side and by dp_add
        return _linear_seq_weight_factor(s, z)

    return {"V_mat_prod": V_mat_prod, "V_t_mat_prod": V_t_mat_prod, "gram_mat": gram_mat, "factor": factor,
            "shape_cn": (C, N), "dp_add": lambda acc: _materialised_closures(factor())["dp_add"](acc)}


def _embedding_closures(M: Tensor, idx: Tensor, module):
    """Closures for an Embedding weight on the compact form ``(B, ids)`` of :func:`_embedding_compact`: the factor
    ``V_t[c, n, w, :] = sum_{t: idx[n, t] = w} M[c, n, t, :]`` ([C, N, num_embeddings, D], at most T non-zero rows per (c, n)) exists
    only when ``factor()`` or ``dp_add`` ask for it.

    Gram: ``kernels.embedding_gram``, the products of the rows of samples that share a token; products: ``kernels.embedding_vmp`` /
    ``embedding_vtmp``.  Non-HIP or non-fp32 tensors: the same formulas in plain torch (a masked einsum, ``index_add_``).
    """
    B, ids = _embedding_compact(module, M, idx)
    C, N, T, D = B.shape
    W = module.num_embeddings
    hip = B.is_cuda and B.dtype == torch.float32

    def gram_mat(out=None, beta=0.0):
        if hip:
            out2d = None if out is None else out.view(C * N, C * N)
            return kernels.embedding_gram(B, ids, out=out2d, alpha=1.0, beta=beta).view(C, N, C, N)
        same = (ids.view(N, T, 1, 1) == ids.view(1, 1, N, T)) & (ids.view(N, T, 1, 1) >= 0)
        G = torch.einsum("cnud,emkd,numk->cnem", B, B, same.to(B.dtype)).contiguous()
        if out is None:
            return G
        out.copy_(G + beta * out if beta != 0.0 else G)
        return out

    def factor():  # the explicit V_t; only asked for by the parameter side
        return _embedding_factor(B, ids, W)

    def V_mat_prod(mat):  # [F, C, N] -> [F, W, D]
        return kernels.embedding_vmp(B, ids, mat, W) if hip else Vmp(factor(), mat, 2)

    def V_t_mat_prod(mat):  # [F, W, D] -> [F, C, N]
        return kernels.embedding_vtmp(B, ids, mat) if hip else mVp(factor(), mat, 2)

    return {"V_mat_prod": V_mat_prod, "V_t_mat_prod": V_t_mat_prod, "gram_mat": gram_mat, "factor": factor,
            "shape_cn": (C, N), "dp_add": lambda acc: _materialised_closures(factor())["dp_add"](acc)}


class _ViViTGGN(_SqrtGGN):
    """Functional access to ``V``, ``V^T`` and the Gram matrix
    (vivit/extensions/secondorder/vivit/__init__.py:63-133)."""

    def _store(self, module, name, param, M, x, subsampling=None):
        if isinstance(module, nn.Linear) and name == "weight" and M.dim() == 3:
            closures = _linear_weight_closures(M, x)
        elif (isinstance(module, nn.Linear) and name == "weight" and M.dim() > 3 and M.is_cuda and M.dtype == torch.float32
              and 4 * M.shape[0] * M.shape[1] * module.out_features * module.in_features > SEQ_LINEAR_EXPLICIT_MAX_BYTES):
            closures = _linear_seq_weight_closures(M, x)
        elif isinstance(module, nn.Embedding):
            closures = _embedding_closures(M, x, module)
        else:
            closures = _materialised_closures(_param_factor_of(module, name, M, x, subsampling))
        setattr(param, self.savefield, closures)


class ViViTGGNExact(_ViViTGGN):
    savefield = "vivit_ggn_exact"
    strategy = "exact"

    def __init__(self, subsampling=None):
        super().__init__(subsampling)


class ViViTGGNMC(_ViViTGGN):
    savefield = "vivit_ggn_mc"
    strategy = "sampling"

    def __init__(self, mc_samples: int = 1, subsampling=None, samples: Optional[Tensor] = None):
        super().__init__(subsampling, mc_samples, samples)
