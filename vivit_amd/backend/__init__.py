"""Self-contained stand-in for the BackPACK protocol the ViViT hooks are driven by.

``backpack-for-pytorch`` (>=1.5,<2; reference setup.cfg:36) is not available on the build or the
GPU box, so the boundary the path sits behind -- ``extend(model)``, ``with backpack(*extensions,
extension_hook=hook): loss.backward()``, quantities attached to parameters under an
extension's ``savefield``, ``hook(module)`` called per module after its extensions ran -- is
provided here for feed-forward and residual nets (Linear, Conv1d/2d/3d, ConvTranspose1d/2d/3d, BatchNorm in
eval mode, element-wise activations, pooling, Flatten, Dropout in eval mode, and the branching modules
``Parallel`` / ``SumModule`` / ``Pad`` / ``Slicing`` / ``ScaleModule`` of ``backpack.custom_module``, LayerNorm / GroupNorm,
the self-attention modules ``ScaledDotProductAttention`` / ``MultiheadSelfAttention`` of ``custom_module`` (causal,
grouped queries, sliding windows, right-padded batches through ``set_lengths``, logit soft-capping and relative-position
bias tables, constant such as ``alibi_bias`` or learned, plain or indexed through ``relative_position_buckets``; ``SoftCap`` for capped final logits), the cross-attention modules
``ScaledDotProductCrossAttention`` / ``MultiheadCrossAttention`` (queries over a second sequence), ``nn.Embedding``,
``nn.RMSNorm`` and the modules ``ProductModule`` (gated MLPs) / ``RotaryEmbedding`` of ``custom_module``;
CrossEntropyLoss / MSELoss with ``reduction='mean'`` or ``'sum'``, on outputs ``[N, C]`` and on outputs with positions
``[N, C, *D]`` -- next-token cross entropy over a whole sequence, segmentation, dense regression -- with ``Permute`` of
``custom_module`` to bring a head's ``[N, T, C]`` to ``[N, C, T]``).  When the real BackPACK is importable the Computation classes can be used
with it directly; this module is never imported in that case.

This is the FACTOR PROVIDER, i.e. the producer of the path's inputs
(``V_t``, ``grad_batch``), not the measured hot path; it uses torch ops for the per-layer
Jacobian rules and the HIP kernels only where a rule is GEMM-shaped.
"""
from vivit_amd.backend.custom_module import (
    ActiveIdentity,
    MultiheadCrossAttention,
    MultiheadSelfAttention,
    Pad,
    Parallel,
    Permute,
    ProductModule,
    RotaryEmbedding,
    ScaledDotProductAttention,
    ScaledDotProductCrossAttention,
    ScaleModule,
    Slicing,
    SoftCap,
    SumModule,
    alibi_bias,
    relative_position_buckets,
)
from vivit_amd.backend.engine import backpack, extend
from vivit_amd.backend.extensions import (
    BatchGrad,
    SqrtGGNExact,
    SqrtGGNMC,
    ViViTGGNExact,
    ViViTGGNMC,
)

__all__ = ["ActiveIdentity", "MultiheadCrossAttention", "MultiheadSelfAttention", "Pad", "Parallel", "Permute", "ProductModule", "RotaryEmbedding", "ScaledDotProductAttention", "ScaledDotProductCrossAttention", "ScaleModule", "Slicing", "SoftCap", "SumModule", "alibi_bias", "relative_position_buckets", "backpack", "extend", "BatchGrad", "SqrtGGNExact", "SqrtGGNMC", "ViViTGGNExact", "ViViTGGNMC"]
