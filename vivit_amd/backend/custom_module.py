"""Branching / padding / slicing / scaling modules of the stand-in backend.

Counterparts of ``backpack.custom_module.{branching,pad,slicing,scale_module}`` which the reference's ViViT extensions
support (vivit/extensions/secondorder/vivit/__init__.py:113-117) and its tests use for skip connections
(test/settings.py:161-181): residual networks are written as ``Parallel(branch_1, ..., branch_k)`` whose outputs a
``SumModule`` adds, so that every tensor operation belongs to a leaf module the extensions can differentiate.
"""
from typing import Sequence, Tuple, Union

import math

import torch
from torch import Tensor, nn
from torch.nn import functional as F


class SumModule(nn.Module):
    """Sum of its inputs (``backpack.custom_module.branching.SumModule``)."""

    def forward(self, *inputs: Tensor) -> Tensor:
        out = inputs[0]
        for t in inputs[1:]:
            out = out + t
        return out if len(inputs) > 1 else out * 1.0


class ProductModule(nn.Module):
    """Elementwise product of exactly two inputs of equal shape (no counterpart in BackPACK): the merge of a gated MLP,
    ``Parallel(Sequential(Linear, SiLU), Linear, merge_module=ProductModule())`` is SwiGLU's ``silu(x W1) * (x W3)``."""

    def forward(self, *inputs: Tensor) -> Tensor:
        if len(inputs) != 2:
            raise ValueError(f"ProductModule multiplies exactly two inputs, got {len(inputs)}")
        a, b = inputs
        if a.shape != b.shape:
            raise ValueError(f"ProductModule needs inputs of equal shape, got {tuple(a.shape)} and {tuple(b.shape)}")
        return a * b


class ActiveIdentity(nn.Module):
    """Identity that produces a new tensor (``backpack.custom_module.branching.ActiveIdentity``)."""

    def forward(self, x: Tensor) -> Tensor:
        return x * 1.0


class Parallel(nn.Module):
    """Feed the input to every branch, merge the results (``backpack.custom_module.branching.Parallel``)."""

    def __init__(self, *branches: nn.Module, merge_module: nn.Module = None):
        super().__init__()
        for i, b in enumerate(branches):
            self.add_module(f"branch{i}", b)
        self._num = len(branches)
        self.merge = SumModule() if merge_module is None else merge_module

    def forward(self, x: Tensor) -> Tensor:
        return self.merge(*[getattr(self, f"branch{i}")(x) for i in range(self._num)])


class Pad(nn.Module):
    """``torch.nn.functional.pad`` as a module (``backpack.custom_module.pad.Pad``)."""

    def __init__(self, pad: Sequence[int], mode: str = "constant", value: float = 0.0):
        super().__init__()
        self.pad, self.mode, self.value = tuple(pad), mode, value

    def forward(self, x: Tensor) -> Tensor:
        return F.pad(x, self.pad, mode=self.mode, value=self.value)


class Slicing(nn.Module):
    """``x[slice_info]`` as a module (``backpack.custom_module.slicing.Slicing``)."""

    def __init__(self, slice_info: Tuple[Union[slice, int], ...]):
        super().__init__()
        self.slice_info = slice_info

    def forward(self, x: Tensor) -> Tensor:
        return x[self.slice_info]


class Permute(nn.Module):
    """``x.permute(dims)`` as a module (``backpack.custom_module.permute.Permute``); the batch axis stays in front
    (``dims[0] == 0``).  ``Permute(0, 2, 1)`` takes a head's ``[N, T, C]`` to the ``[N, C, T]`` that ``nn.CrossEntropyLoss`` wants."""

    def __init__(self, *dims: int):
        super().__init__()
        if len(dims) == 1 and isinstance(dims[0], (tuple, list)):
            dims = tuple(dims[0])
        if not all(isinstance(d, int) for d in dims) or sorted(dims) != list(range(len(dims))):
            raise ValueError(f"dims must be a permutation of 0 .. {len(dims) - 1}, got {dims}")
        if not dims or dims[0] != 0:
            raise ValueError(f"the batch axis must stay in front (dims[0] == 0), got {dims}")
        self.dims = tuple(dims)

    def inverse_dims(self) -> Tuple[int, ...]:
        inv = [0] * len(self.dims)
        for i, d in enumerate(self.dims):
            inv[d] = i
        return tuple(inv)

    def forward(self, x: Tensor) -> Tensor:
        return x.permute(self.dims)


class ScaleModule(nn.Module):
    """``x * weight`` with a constant scalar (``backpack.custom_module.scale_module.ScaleModule``)."""

    def __init__(self, weight: float = 1.0):
        super().__init__()
        self.weight = float(weight)

    def forward(self, x: Tensor) -> Tensor:
        return x * self.weight


def _kv_heads(num_heads: int, num_kv_heads):
    """The ``num_kv_heads`` argument of the attention modules, validated (``None`` stays ``None``: multi-head attention)."""
    if num_kv_heads is None:
        return None
    if num_kv_heads < 1:
        raise ValueError(f"num_kv_heads (Hkv) must be positive, got {num_kv_heads}")
    if num_heads % num_kv_heads != 0:
        raise ValueError(f"num_heads (H = {num_heads}) is not a multiple of num_kv_heads (Hkv = {num_kv_heads})")
    return int(num_kv_heads)


def _head_dim(qkv: Tensor, H: int, num_kv_heads, even: bool = False) -> int:
    """The head dimension ``d`` of a packed projection ``qkv [N, T, (H + 2 Hkv) d]``, checked (``even``: and even).  Without
    ``num_kv_heads`` (``Hkv = H``) the messages speak of the three thirds ``[N, T, 3 E]``."""
    if num_kv_heads is None:
        heads, layout, count = 3 * H, "3 E", f"3 * {H}"
    else:
        heads, layout, count = H + 2 * num_kv_heads, "(H + 2 Hkv) d", f"(H + 2 Hkv) = ({H} + 2 * {num_kv_heads})"
    if qkv.dim() != 3:
        raise ValueError(f"expected a packed projection [N, T, {layout}], got {qkv.dim()} dimensions")
    if qkv.shape[2] == 0 or qkv.shape[2] % heads != 0:
        raise ValueError(f"the last dimension ({qkv.shape[2]}) is not {count} heads * head dimension")
    d = qkv.shape[2] // heads
    if even and d % 2 != 0:
        raise ValueError(f"the head dimension ({d}) must be even: rotary embeddings rotate pairs of columns")
    return d


def _gqa_split(x: Tensor, H: int, Hkv: int, d: int) -> Tuple[Tensor, Tensor, Tensor]:
    """Views of a packed projection ``x [*B, T, (H + 2 Hkv) d]``: ``q [*B, Hkv, R, T, d]`` and ``k``, ``v [*B, Hkv, 1, T, d]``."""
    nb = x.dim() - 2
    heads = lambda t, R: t.unflatten(-2, (Hkv, R)).permute(*range(nb), nb + 1, nb + 2, nb, nb + 3)   # noqa: E731
    # (one split of the head axis, not three slices of the columns: its gradient is one concatenation of the three gradients as they
    # come, where each slice's is a zero-filled copy to be added up)
    q, k, v = x.unflatten(-1, (H + 2 * Hkv, d)).split((H, Hkv, Hkv), -2)
    return heads(q, H // Hkv), heads(k, 1), heads(v, 1)


def _window(window):
    """The ``window`` argument of the attention modules, validated (``None`` stays ``None``: no window)."""
    if window is None:
        return None
    if isinstance(window, bool) or int(window) != window or window < 1:
        raise ValueError(f"window must be an integer >= 1 (or None), got {window!r}")
    return int(window)


def attention_visible(T: int, lengths, causal: bool, window, device) -> Tensor:
    """The boolean mask ``[N, T, T]`` (``[1, T, T]`` without lengths) of the attention modules' forward pass: query ``i`` of sample
    ``n`` sees key ``j`` iff ``i, j < lengths[n]``, ``j <= i`` when ``causal`` and ``|i - j| < window`` when a window is given.  A dead
    query (``i >= lengths[n]``) is given its own position to look at, so that no row of the softmax is empty: its value row is zero
    (the forward pass zeroes the dead rows of its input), and so is its output."""
    t = torch.arange(T, device=device)
    dist = t[:, None] - t[None, :]                                          # i - j
    vis = torch.ones(1, T, T, dtype=torch.bool, device=device)
    if causal:
        vis = vis & (dist >= 0)
    if window is not None:
        vis = vis & (dist.abs() < window)
    if lengths is not None:
        live = t[None, :] < lengths.to(device)[:, None]                     # [N, T]
        vis = (vis & live[:, :, None] & live[:, None, :]) | (dist == 0)
    return vis


def _softcap(cap):
    """The ``softcap`` argument of the attention modules and of :class:`SoftCap`, validated (``None`` stays ``None``: no cap)."""
    if cap is None:
        return None
    if isinstance(cap, bool) or not isinstance(cap, (int, float)) or not (cap > 0) or math.isinf(cap):
        raise ValueError(f"softcap must be a finite float > 0 (or None), got {cap!r}")
    return float(cap)


class SoftCap(nn.Module):
    """``cap * tanh(x / cap)`` (no counterpart in BackPACK): the soft cap of Gemma-2's and Grok-1's final logits, an elementwise
    leaf (the rule is the activation kind ``"softcap"`` of ``kernels.act_jac_t``)."""

    def __init__(self, cap: float):
        super().__init__()
        if cap is None:
            raise ValueError("SoftCap needs a cap")
        self.cap = _softcap(cap)

    def forward(self, x: Tensor) -> Tensor:
        return self.cap * torch.tanh(x / self.cap)

    def extra_repr(self) -> str:
        return f"cap={self.cap}"


def _bias_index(index) -> Tensor:
    """The ``bias_index`` argument of the attention modules, validated: an integer tensor ``[2 L - 1]`` of values ``>= 0``."""
    if not isinstance(index, Tensor) or index.is_floating_point() or index.is_complex() or index.dtype == torch.bool:
        raise ValueError(f"bias_index must be an integer tensor [2 L - 1], got "
                         f"{index.dtype if isinstance(index, Tensor) else type(index).__name__}")
    if index.dim() != 1 or index.shape[0] % 2 != 1:
        raise ValueError(f"bias_index must be [2 L - 1] (an odd width), got {tuple(index.shape)}")
    if int(index.min()) < 0:
        raise ValueError(f"bias_index must lie in [0, R), got {int(index.min())}")
    return index.detach().clone().to(torch.int64)


def relative_position_buckets(max_len: int, num_buckets: int = 32, max_distance: int = 128, bidirectional: bool = True) -> Tensor:
    """T5's bucket of every relative position (Raffel et al., 2020) for ``ScaledDotProductAttention(bias_index=...)``: int64
    ``[2 max_len - 1]``, entry ``r + max_len - 1`` is the bucket of the distance ``r = j - i`` (key minus query).  Bidirectional:
    half the buckets serve ``r > 0``, the other half ``r <= 0``; otherwise every ``r > 0`` shares bucket 0 with ``r = 0``.  Within a
    half the first ``max_exact = half // 2`` distances have a bucket each, the rest share logarithmically spaced buckets up to
    ``max_distance``, beyond which all fall into the last.  The logarithm is taken in float32, as T5's implementation does."""
    if max_len < 1:
        raise ValueError(f"max_len must be positive, got {max_len}")
    if num_buckets < (4 if bidirectional else 2) or max_distance < 2:
        raise ValueError(f"num_buckets ({num_buckets}) and max_distance ({max_distance}) are too small for a logarithmic range")
    r = torch.arange(-(max_len - 1), max_len, dtype=torch.int64)
    offset = torch.zeros_like(r)
    if bidirectional:
        num_buckets //= 2
        offset = (r > 0).to(torch.int64) * num_buckets
        r = r.abs()
    else:
        r = (-r).clamp(min=0)
    max_exact = num_buckets // 2
    if max_distance <= max_exact:
        raise ValueError(f"max_distance ({max_distance}) must exceed the exact range ({max_exact})")
    far = r.clamp(min=1).to(torch.float32)    # (the clamp only keeps log(0) out of the entries r < max_exact, which do not use it)
    far = max_exact + (torch.log(far / max_exact) / math.log(max_distance / max_exact) * (num_buckets - max_exact)).to(torch.int64)
    far = far.clamp(max=num_buckets - 1)
    return offset + torch.where(r < max_exact, r, far)


def alibi_slopes(num_heads: int) -> Tensor:
    """The head slopes ``m_h`` of ALiBi (Press et al., 2022) in float64: for ``H`` a power of two the geometric sequence
    ``2^(-8 (h + 1) / H)``; for another ``H`` the slopes of the next lower power of two ``P``, then every second slope of ``2 P``
    (the first, third, ... of that sequence) until there are ``H``."""
    if num_heads < 1:
        raise ValueError(f"num_heads must be positive, got {num_heads}")
    geometric = lambda n: [2.0 ** (-8.0 * (h + 1) / n) for h in range(n)]   # noqa: E731
    P = 1 << (int(num_heads).bit_length() - 1)
    slopes = geometric(P)
    if P < num_heads:
        slopes += geometric(2 * P)[0::2][:num_heads - P]
    return torch.tensor(slopes, dtype=torch.float64)


def alibi_bias(num_heads: int, max_len: int) -> Tensor:
    """The ALiBi table for ``ScaledDotProductAttention(bias=...)``: ``[H, 2 max_len - 1]`` float32, entry ``[h, j - i + max_len - 1]``
    is ``-m_h |j - i|`` with the slopes of :func:`alibi_slopes`.  Under ``causal`` only the half ``j <= i`` is ever read."""
    if max_len < 1:
        raise ValueError(f"max_len must be positive, got {max_len}")
    dist = torch.arange(-(max_len - 1), max_len, dtype=torch.float64).abs()
    return (-alibi_slopes(num_heads)[:, None] * dist[None, :]).to(torch.float32)


class ScaledDotProductAttention(nn.Module):
    """Multi-head scaled dot-product self-attention on a packed projection (no counterpart in BackPACK): a leaf whose one possible parameter is a
    learned bias table (``learn_bias``, below).

    Input ``qkv [N, T, 3 E]`` with ``q = qkv[..., :E]``, ``k = qkv[..., E:2 E]``, ``v = qkv[..., 2 E:]``; head ``h`` owns the columns
    ``h d .. (h + 1) d`` of each third (``d = E / num_heads``, the layout of ``nn.MultiheadAttention``'s packed projection).  Output
    ``[N, T, E]``: per head ``softmax(scale q k^T) v`` with ``scale = 1 / sqrt(d)`` by default; ``causal`` masks the keys ``j > i``.
    No dropout.  ``window`` (an integer ``>= 1``; sliding-window attention): query ``i`` sees the keys with ``|i - j| < window`` --
    with ``causal`` the ``window`` keys ``i - window + 1 .. i``, its own position included (Mistral's convention); ``window >= T`` is
    no window.  No arbitrary ``[T, T]`` or per-sample mask.

    Score modifiers.  With ``z_ij = scale q_i k_j`` the logits are ``s_ij = u_ij + bias[h, j - i + L - 1]``, ``u = softcap *
    tanh(z / softcap)``, then the mask: the cap comes before the bias, and both before the mask (Gemma-2's order).  ``softcap`` (a
    finite float ``> 0``; ``None``: ``u = z``) is the logit cap of Gemma-2 and Grok-1.  ``bias`` (``None``: none) is a tensor
    ``[H, 2 L - 1]`` for a maximum length ``L``: one value per query head and distance ``j - i``, as ALiBi (:func:`alibi_bias`) and
    the relative-position tables of T5 and Swin have it.  A batch of ``T <= L`` positions uses the middle slice
    ``bias[:, L - T : L + T - 1]``; ``T > L`` is a ``ValueError``.  The table is a buffer of the module (it moves with ``.to()``) and
    a constant of the function, unless ``learn_bias=True``: the table is then an ``nn.Parameter`` of the same name (the
    ``state_dict`` keys stay the same), autograd reaches it through the forward pass, and the extensions give it its own factor
    ``[V, N, *bias.shape]`` (the diagonal sums of ``dS``: ``kernels.attention_bias_factor``).  Its entries must be finite; that is
    checked at construction only, the forward pass never reads the table on the host.  ``bias_index`` (an integer tensor
    ``[2 L - 1]`` with values in ``[0, R)``; a buffer) indexes the table through buckets, as T5 does: the table is then ``bias [H, R]``
    and distance ``j - i`` reads ``bias[h, bias_index[j - i + L - 1]]`` -- many distances share one entry
    (:func:`relative_position_buckets`).

    Padded batches: ``set_lengths(lengths)`` gives sample ``n`` the positions ``0 .. lengths[n] - 1`` (RIGHT padding only; a
    left-padded batch is not supported) for every forward pass until it is reset with ``set_lengths(None)``.  The positions beyond are
    dead, the convention of variable-length attention kernels and not that of ``key_padding_mask``: as keys they are invisible, as
    queries their output row is exact zeros, nothing flows back to them, and whatever the input holds there (NaN included) reaches
    no live position.  A live query always sees itself, so no row of the softmax is empty.  ``lengths`` is a sequence or an integer
    tensor ``[N]``: one on the host is checked to lie in ``[0, T]`` at the next forward pass; one on a device is never read on the
    host and is clamped to ``[0, T]``, as the kernel of the extensions' rule clamps it.  The forward pass keeps the int32 tensor it
    used on the module (``forward_lengths``), and the rule reads that one: the very lengths of the forward pass.

    ``num_kv_heads`` (grouped-query attention; ``None``: every query head has its own key and value head): the ``H = num_heads``
    query heads share ``Hkv = num_kv_heads`` key / value heads, ``H % Hkv == 0``.  Input ``qkv [N, T, (H + 2 Hkv) d]``: ``q`` is the
    first ``H d`` columns, ``k`` the next ``Hkv d``, ``v`` the last ``Hkv d``; query head ``h`` attends to key / value head
    ``h // (H / Hkv)`` (groups of consecutive heads, as LLaMA's ``repeat_kv``).  Output ``[N, T, H d]``.  ``Hkv == 1`` is multi-query
    attention."""

    def __init__(self, num_heads: int, causal: bool = False, scale: float = None, num_kv_heads: int = None, window: int = None,
                 softcap: float = None, bias: Tensor = None, learn_bias: bool = False, bias_index: Tensor = None):
        super().__init__()
        if num_heads < 1:
            raise ValueError(f"num_heads must be positive, got {num_heads}")
        if bias is None and learn_bias:
            raise ValueError("learn_bias=True needs a bias table to learn")
        if bias is None and bias_index is not None:
            raise ValueError("bias_index indexes a bias table: give one")
        if bias_index is not None:
            bias_index = _bias_index(bias_index)
        self.num_heads, self.causal, self.scale = int(num_heads), bool(causal), scale
        self.num_kv_heads = _kv_heads(num_heads, num_kv_heads)
        self.window = _window(window)
        self.softcap = _softcap(softcap)
        if bias is not None:
            if not isinstance(bias, Tensor) or not bias.is_floating_point() or bias.dim() != 2 or bias.shape[0] != num_heads or \
                    (bias_index is None and bias.shape[1] % 2 != 1) or bias.shape[1] < 1:
                raise ValueError(f"bias must be a floating-point tensor [H = {num_heads}, {'2 L - 1' if bias_index is None else 'R'}], got "
                                 f"{tuple(bias.shape) if isinstance(bias, Tensor) else type(bias).__name__}")
            if bias_index is not None and int(bias_index.max()) >= bias.shape[1]:
                raise ValueError(f"bias_index reaches entry {int(bias_index.max())}, the bias table [H, R] has R = {bias.shape[1]}")
            if not bool(torch.isfinite(bias).all()):
                raise ValueError("bias must be finite (masking is what causal, window and set_lengths are for)")
            bias = bias.detach().clone()
        self.learn_bias = bool(learn_bias)
        if self.learn_bias:
            self.bias = nn.Parameter(bias)
        else:
            self.register_buffer("bias", bias)
        self.register_buffer("bias_index", bias_index)
        self._lengths = None          # what set_lengths() was given
        self.forward_lengths = None   # int32 [N] on the input's device: what the last forward() used (None: no lengths)

    def set_lengths(self, lengths) -> None:
        """Per-sample sequence lengths of the batches to come (``None``: none); see the class docstring."""
        if lengths is not None:
            lengths = torch.as_tensor(lengths)
            if lengths.dim() != 1 or lengths.is_floating_point() or lengths.is_complex() or lengths.dtype == torch.bool:
                raise ValueError(f"lengths must be integers [N], got {lengths.dtype} {tuple(lengths.shape)}")
        self._lengths = lengths

    def lengths_for(self, qkv: Tensor):
        """The lengths of set_lengths() for the batch ``qkv`` as int32 on its device, checked (on the host only) against it."""
        if self._lengths is None:
            return None
        N, T = qkv.shape[:2]
        if self._lengths.shape[0] != N:
            raise ValueError(f"set_lengths() was given {self._lengths.shape[0]} lengths, the batch has {N} samples")
        if self._lengths.device.type == "cpu" and N > 0 and (int(self._lengths.min()) < 0 or int(self._lengths.max()) > T):
            raise ValueError(f"lengths must lie in [0, T = {T}], got {self._lengths.tolist()}")
        return self._lengths.to(device=qkv.device, dtype=torch.int32)

    @property
    def kv_heads(self) -> int:
        """``Hkv``: ``num_kv_heads``, or ``num_heads`` where none was given (multi-head attention is ``Hkv = H``)."""
        return self.num_heads if self.num_kv_heads is None else self.num_kv_heads

    def head_dim(self, qkv: Tensor) -> int:
        return _head_dim(qkv, self.num_heads, self.num_kv_heads)

    def scale_for(self, d: int) -> float:
        return float(self.scale) if self.scale is not None else d ** -0.5

    def bias_max_len(self) -> int:
        """``L``: the most positions the table (through its index, where it has one) was built for."""
        return ((self.bias.shape[1] if self.bias_index is None else self.bias_index.shape[0]) + 1) // 2

    def bias_columns(self, T: int, device=None) -> Tensor:
        """Where the distances of a batch of ``T`` positions sit in the table: integers ``[2 T - 1]``, entry ``j - i + T - 1`` is the
        column of ``bias`` that distance reads -- the middle slice of ``bias_index``, or ``k + (L - T)`` for a plain table."""
        L = self.bias_max_len()
        if T > L:
            raise ValueError(f"the batch has T = {T} positions, the bias table was built for at most {L}")
        if self.bias_index is None:
            return torch.arange(L - T, L + T - 1, device=self.bias.device if device is None else device)
        return self.bias_index[L - T:L + T - 1]

    def bias_for(self, T: int):
        """The table of a batch of ``T`` positions, ``[H, 2 T - 1]`` indexed by ``j - i + T - 1`` (without an index a view: the middle
        slice of the table; with one ``bias[:, bias_index]``'s middle slice); ``None`` without a table."""
        if self.bias is None:
            return None
        L = self.bias_max_len()
        if T > L:
            raise ValueError(f"the batch has T = {T} positions, the bias table was built for at most {L}")
        if self.bias_index is not None:
            return self.bias[:, self.bias_index[L - T:L + T - 1]]
        return self.bias[:, L - T:L + T - 1]

    def modify(self, z: Tensor) -> Tensor:
        """The logits ``s [N, Hkv, R, T, T]`` before the mask from ``z = scale q k^T``: the cap, then the bias."""
        T = z.shape[-1]
        if self.softcap is not None:
            z = self.softcap * torch.tanh(z / self.softcap)
        table = self.bias_for(T)
        if table is not None:
            t = torch.arange(T, device=z.device)
            z = z + table.to(z.dtype)[:, t[None, :] - t[:, None] + (T - 1)].view(z.shape[-4], z.shape[-3], T, T)
        return z

    def forward(self, qkv: Tensor) -> Tensor:
        self.head_dim(qkv)
        self.bias_for(qkv.shape[1])
        self.forward_lengths = self.lengths_for(qkv)
        return self.attend(qkv, self.forward_lengths)

    def masks(self, T: int, lengths, device):
        """``(hidden, dead)`` for ``T`` positions and ``lengths`` (int32 ``[N]`` on ``device``, or ``None``).  ``hidden``: the pairs
        (query, key) that do not see each other, ``[T, T]`` (the causal mask alone) or ``[N | 1, 1, 1, T, T]``, either of which
        broadcasts over the scores ``[N, Hkv, R, T, T]``; ``None``: every pair sees each other.  ``dead``: the positions
        ``t >= lengths[n]``, ``[N, T, 1]``; ``None`` without lengths."""
        hidden = dead = None
        if lengths is not None or self.window is not None:
            hidden = ~attention_visible(T, lengths, self.causal, self.window, device)[:, None, None]
            if lengths is not None:
                dead = (torch.arange(T, device=device)[None, :] >= lengths[:, None])[:, :, None]
        elif self.causal:
            hidden = torch.ones(T, T, dtype=torch.bool, device=device).triu(1)
        return hidden, dead

    def attend(self, qkv: Tensor, lengths) -> Tensor:
        """The forward pass with explicit ``lengths`` (int32 ``[N]`` on the device of ``qkv``, or ``None``)."""
        d = self.head_dim(qkv)
        N, T, H = qkv.shape[0], qkv.shape[1], self.num_heads
        hidden, dead = self.masks(T, lengths, qkv.device)
        if dead is not None:   # the dead rows of q, k and v are zeros, whatever the input holds there
            qkv = qkv.masked_fill(dead, 0.0)
        q, k, v = _gqa_split(qkv, H, self.kv_heads, d)                    # q [N, Hkv, R, T, d]; k, v [N, Hkv, 1, T, d]: views
        s = self.modify((q @ k.transpose(-1, -2)) * self.scale_for(d))    # (the matmul broadcasts k and v over the group)
        if hidden is not None:
            s = s.masked_fill(hidden, float("-inf"))
        return (s.softmax(-1) @ v).reshape(N, H, T, d).transpose(1, 2).reshape(N, T, H * d)   # (a new tensor: the heads are gathered)


class RotaryEmbedding(nn.Module):
    """Rotary position embedding on a packed projection ``qkv [N, T, 3 E]`` (no counterpart in BackPACK): a parameter-free leaf
    in front of :class:`ScaledDotProductAttention`, whose layout it shares (head ``h`` owns the columns ``h d .. (h + 1) d`` of each
    third, ``d = E / num_heads``, which must be even).

    Half-split pairing ("rotate_half", as LLaMA / GPT-NeoX): in every head of the q and k thirds the pair ``(j, j + d / 2)`` at
    position ``t`` is rotated by the angle ``t * base^(-2 j / d)``, ``y1 = x1 cos - x2 sin``, ``y2 = x2 cos + x1 sin``; the v third
    passes through.  Positions start at 0.

    ``num_kv_heads`` (grouped-query attention, as :class:`ScaledDotProductAttention`): ``qkv [N, T, (H + 2 Hkv) d]``; the ``H`` query
    heads and the ``Hkv`` key heads are rotated, the ``Hkv d`` columns of v pass through."""

    def __init__(self, num_heads: int, base: float = 10000.0, num_kv_heads: int = None):
        super().__init__()
        if num_heads < 1:
            raise ValueError(f"num_heads must be positive, got {num_heads}")
        self.num_heads, self.base = int(num_heads), float(base)
        self.num_kv_heads = _kv_heads(num_heads, num_kv_heads)
        self._tables = None   # (key, cos, sin): what forward() used is what the rule of the extensions uses

    @property
    def kv_heads(self) -> int:
        """``Hkv``: ``num_kv_heads``, or ``num_heads`` where none was given (three equal thirds are ``Hkv = H``)."""
        return self.num_heads if self.num_kv_heads is None else self.num_kv_heads

    def head_dim(self, qkv: Tensor) -> int:
        return _head_dim(qkv, self.num_heads, self.num_kv_heads, even=True)

    def tables(self, T: int, d: int, device, dtype) -> Tuple[Tensor, Tensor]:
        """``(cos, sin)``, each ``[T, d / 2]`` in ``dtype``: the angles ``t * base^(-2 j / d)`` are computed in fp32 and the tables
        cached on the module, so that every caller with the same arguments gets the same tensors."""
        key = (int(T), int(d), torch.device(device), dtype, self.base)
        if self._tables is None or self._tables[0] != key:
            j = torch.arange(d // 2, dtype=torch.float32, device=device)
            inv_freq = self.base ** (-2.0 * j / d)
            angle = torch.arange(T, dtype=torch.float32, device=device)[:, None] * inv_freq[None, :]
            self._tables = (key, angle.cos().to(dtype), angle.sin().to(dtype))
        return self._tables[1], self._tables[2]

    def forward(self, qkv: Tensor) -> Tensor:
        d = self.head_dim(qkv)
        N, T, half = qkv.shape[0], qkv.shape[1], d // 2
        rotated = self.num_heads + self.kv_heads   # q | k is H + Hkv heads of d columns; the Hkv d columns of v pass through
        cos, sin = (t.view(1, T, 1, half) for t in self.tables(T, d, qkv.device, qkv.dtype))
        x = qkv[..., :rotated * d].view(N, T, rotated, d)
        x1, x2 = x[..., :half], x[..., half:]
        rot = torch.cat((x1 * cos - x2 * sin, x2 * cos + x1 * sin), -1).reshape(N, T, rotated * d)
        return torch.cat((rot, qkv[..., rotated * d:]), -1)


class MultiheadSelfAttention(nn.Sequential):
    """``Linear(E, 3 E)`` -> :class:`ScaledDotProductAttention` -> ``Linear(E, E)``: ``nn.MultiheadAttention(batch_first=True)``
    applied to ``(x, x, x)`` as a container of single-input leaves, which is what the extensions' rules are written for.  With
    ``num_kv_heads`` (grouped-query attention) the first projection is ``Linear(E, (H + 2 Hkv) d)``, ``d = E / H``.  ``window`` and
    ``set_lengths`` are those of :class:`ScaledDotProductAttention` (sliding-window attention; right-padded batches), and so are
    ``softcap`` and ``attention_bias`` (its ``bias``: the table ``[H, 2 L - 1]``, e.g. :func:`alibi_bias`; the name ``bias`` is taken
    by the flag of the two projections, as in ``nn.MultiheadAttention`` -- a TENSOR given as ``bias`` is taken for the table and the
    projections keep their bias vectors).  ``learn_attention_bias`` and ``attention_bias_index`` are the leaf's ``learn_bias`` and
    ``bias_index``: a learned table, and a table indexed through buckets."""

    def __init__(self, embed_dim: int, num_heads: int, bias: Union[bool, Tensor] = True, causal: bool = False, num_kv_heads: int = None,
                 window: int = None, softcap: float = None, attention_bias: Tensor = None, learn_attention_bias: bool = False,
                 attention_bias_index: Tensor = None):
        if embed_dim % num_heads != 0:
            raise ValueError(f"embed_dim ({embed_dim}) is not divisible by num_heads ({num_heads})")
        if isinstance(bias, Tensor):
            if attention_bias is not None:
                raise ValueError("two bias tables: give the table as bias or as attention_bias, not both")
            bias, attention_bias = True, bias
        attention = ScaledDotProductAttention(num_heads, causal=causal, num_kv_heads=num_kv_heads, window=window, softcap=softcap,
                                              bias=attention_bias, learn_bias=learn_attention_bias, bias_index=attention_bias_index)
        packed = (num_heads + 2 * attention.kv_heads) * (embed_dim // num_heads)
        super().__init__(nn.Linear(embed_dim, packed, bias=bias), attention, nn.Linear(embed_dim, embed_dim, bias=bias))

    def set_lengths(self, lengths) -> None:
        """Per-sample sequence lengths of the padded batches to come (``None``: none), handed to the attention leaf."""
        self[1].set_lengths(lengths)

    @classmethod
    def from_torch(cls, mha: nn.MultiheadAttention, causal: bool = False, window: int = None) -> "MultiheadSelfAttention":
        """A copy of ``mha``'s projections (packed rows q | k | v, as ``in_proj_weight`` has them)."""
        if mha.kdim != mha.embed_dim or mha.vdim != mha.embed_dim or mha.in_proj_weight is None:
            raise ValueError("nn.MultiheadAttention with equal q / k / v dimensions is required")
        if not mha.batch_first or mha.bias_k is not None or mha.add_zero_attn or mha.dropout != 0.0:
            raise ValueError("batch_first=True, no dropout, no bias_k / bias_v and no add_zero_attn are required")
        w = mha.in_proj_weight
        new = cls(mha.embed_dim, mha.num_heads, bias=mha.in_proj_bias is not None, causal=causal, window=window).to(device=w.device, dtype=w.dtype)
        with torch.no_grad():
            new[0].weight.copy_(w)
            new[2].weight.copy_(mha.out_proj.weight)
            if mha.in_proj_bias is not None:
                new[0].bias.copy_(mha.in_proj_bias)
                new[2].bias.copy_(mha.out_proj.bias)
        return new


def _checked_lengths(lengths, name: str):
    """A ``set_lengths`` argument as an integer tensor ``[N]`` (``None`` stays ``None``)."""
    if lengths is None:
        return None
    lengths = torch.as_tensor(lengths)
    if lengths.dim() != 1 or lengths.is_floating_point() or lengths.is_complex() or lengths.dtype == torch.bool:
        raise ValueError(f"{name} must be integers [N], got {lengths.dtype} {tuple(lengths.shape)}")
    return lengths


def _lengths_for(lengths, name: str, N: int, T: int, device):
    """``lengths`` of set_lengths() for a batch of ``N`` samples of ``T`` positions as int32 on ``device``, checked on the host only."""
    if lengths is None:
        return None
    if lengths.shape[0] != N:
        raise ValueError(f"set_lengths() was given {lengths.shape[0]} {name}, the batch has {N} samples")
    if lengths.device.type == "cpu" and N > 0 and (int(lengths.min()) < 0 or int(lengths.max()) > T):
        raise ValueError(f"{name} must lie in [0, T = {T}], got {lengths.tolist()}")
    return lengths.to(device=device, dtype=torch.int32)


class ScaledDotProductCrossAttention(nn.Module):
    """Multi-head scaled dot-product attention of queries over a SECOND sequence (no counterpart in BackPACK): a parameter-free leaf
    of two inputs, ``forward(q, kv)``.

    ``q [N, Tq, H d]`` (head ``h`` owns the columns ``h d .. (h + 1) d``) and ``kv [N, Tk, 2 Hkv d]`` = k | v: ``Hkv`` key heads of
    ``d`` columns, then ``Hkv`` value heads -- the packed layout of :class:`ScaledDotProductAttention` without its query part.
    ``num_kv_heads`` (``None``: ``Hkv = H``): query head ``h`` attends to key / value head ``h // (H / Hkv)``.  Output ``[N, Tq, H d]``:
    per head ``softmax(scale q k^T) v`` with ``scale = 1 / sqrt(d)`` by default.

    NOT supported: no causal mask and no window (with ``Tq != Tk`` there is no agreed alignment of the diagonal), no dropout, no
    arbitrary or additive mask.

    Padded batches: ``set_lengths(query_lengths, key_lengths)`` gives sample ``n`` the queries ``0 .. query_lengths[n] - 1`` and the
    keys ``0 .. key_lengths[n] - 1`` (RIGHT padding only; either may be ``None``: every position) for every forward pass until it is
    reset.  Key ``j`` is live iff ``j < key_lengths[n]``; query ``i`` is live iff ``i < query_lengths[n]`` AND ``key_lengths[n] > 0``:
    a query with no key to look at is dead, it is not a NaN.  Dead keys are invisible, the output rows of dead queries are exact
    zeros, nothing flows back to a dead position, and whatever the inputs hold there (NaN included) reaches no live position.  The
    softmax has no empty row: a dead query is given key 0 to look at (on zeroed data), and its output row is set to zero.  Lengths
    are a sequence or an integer tensor ``[N]``: one on the host is checked to lie in ``[0, Tq]`` / ``[0, Tk]`` at the next forward
    pass; one on a device is never read on the host and is clamped, as the kernel of the extensions' rule clamps it.  The forward
    pass keeps the int32 tensors it used on the module (``forward_query_lengths``, ``forward_key_lengths``), and the rule reads
    those: the very lengths of the forward pass."""

    def __init__(self, num_heads: int, scale: float = None, num_kv_heads: int = None):
        super().__init__()
        if num_heads < 1:
            raise ValueError(f"num_heads must be positive, got {num_heads}")
        self.num_heads, self.scale = int(num_heads), scale
        self.num_kv_heads = _kv_heads(num_heads, num_kv_heads)
        self._query_lengths = self._key_lengths = None                  # what set_lengths() was given
        self.forward_query_lengths = self.forward_key_lengths = None    # int32 [N] on the inputs' device: what the last forward() used

    def set_lengths(self, query_lengths=None, key_lengths=None) -> None:
        """Per-sample lengths of the two sequences of the batches to come (``None``: none); see the class docstring."""
        query_lengths = _checked_lengths(query_lengths, "query_lengths")
        self._query_lengths, self._key_lengths = query_lengths, _checked_lengths(key_lengths, "key_lengths")

    @property
    def kv_heads(self) -> int:
        """``Hkv``: ``num_kv_heads``, or ``num_heads`` where none was given."""
        return self.num_heads if self.num_kv_heads is None else self.num_kv_heads

    def head_dim(self, q: Tensor, kv: Tensor) -> int:
        """The head dimension ``d`` of ``q [N, Tq, H d]`` and ``kv [N, Tk, 2 Hkv d]``, checked."""
        H, Hkv = self.num_heads, self.kv_heads
        if q.dim() != 3 or q.shape[2] == 0 or q.shape[2] % H != 0:
            raise ValueError(f"expected queries [N, Tq, H d] with H = {H}, got {tuple(q.shape)}")
        d = q.shape[2] // H
        if kv.dim() != 3 or kv.shape[0] != q.shape[0] or kv.shape[1] == 0 or kv.shape[2] != 2 * Hkv * d:
            raise ValueError(f"expected keys and values [N = {q.shape[0]}, Tk, 2 Hkv d = 2 * {Hkv} * {d}], got {tuple(kv.shape)}")
        return d

    def scale_for(self, d: int) -> float:
        return float(self.scale) if self.scale is not None else d ** -0.5

    def forward(self, q: Tensor, kv: Tensor) -> Tensor:
        self.head_dim(q, kv)
        N, Tq, Tk = q.shape[0], q.shape[1], kv.shape[1]
        self.forward_query_lengths = _lengths_for(self._query_lengths, "query_lengths", N, Tq, q.device)
        self.forward_key_lengths = _lengths_for(self._key_lengths, "key_lengths", N, Tk, q.device)
        return self.attend(q, kv, self.forward_query_lengths, self.forward_key_lengths)

    @staticmethod
    def masks(N: int, Tq: int, Tk: int, query_lengths, key_lengths, device):
        """``(hidden, dead_q, dead_k)`` for lengths given as int32 ``[N]`` on ``device`` or ``None``; three ``None`` without any.
        ``hidden [N, 1, 1, Tq, Tk]``: the pairs (query, key) that do not see each other -- a dead query keeps key 0, so that no row
        is empty; ``dead_q [N, Tq, 1]``, ``dead_k [N, Tk, 1]``: the dead positions."""
        if query_lengths is None and key_lengths is None:
            return None, None, None
        lk = torch.full((N,), Tk, dtype=torch.int32, device=device) if key_lengths is None else key_lengths
        lq = torch.full((N,), Tq, dtype=torch.int32, device=device) if query_lengths is None else query_lengths
        lq = torch.where(lk > 0, lq, torch.zeros_like(lq))              # no key to look at: the queries are dead
        dead_q = torch.arange(Tq, device=device)[None, :] >= lq[:, None]    # [N, Tq]
        dead_k = torch.arange(Tk, device=device)[None, :] >= lk[:, None]    # [N, Tk]
        first = torch.arange(Tk, device=device) == 0
        hidden = torch.where(dead_q[:, :, None], ~first[None, None, :], dead_k[:, None, :])
        return hidden[:, None, None], dead_q[:, :, None], dead_k[:, :, None]

    def split(self, q: Tensor, kv: Tensor, d: int) -> Tuple[Tensor, Tensor, Tensor]:
        """Views ``q [*B, Hkv, R, Tq, d]`` and ``k``, ``v [*B, Hkv, 1, Tk, d]`` of ``q [*B, Tq, H d]`` and ``kv [*B, Tk, 2 Hkv d]``."""
        Hkv, nb = self.kv_heads, q.dim() - 2
        qh = q.unflatten(-1, (Hkv, self.num_heads // Hkv, d)).permute(*range(nb), nb + 1, nb + 2, nb, nb + 3)
        k, v = kv.unflatten(-1, (2 * Hkv, d)).split((Hkv, Hkv), -2)
        heads = lambda t: t.permute(*range(nb), nb + 1, nb, nb + 2).unsqueeze(-3)   # [*B, Tk, Hkv, d] -> [*B, Hkv, 1, Tk, d]  # noqa: E731
        return qh, heads(k), heads(v)

    def attend(self, q: Tensor, kv: Tensor, query_lengths, key_lengths) -> Tensor:
        """The forward pass with explicit lengths (int32 ``[N]`` on the device of the inputs, or ``None``)."""
        d = self.head_dim(q, kv)
        N, Tq, H = q.shape[0], q.shape[1], self.num_heads
        hidden, dead_q, dead_k = self.masks(N, Tq, kv.shape[1], query_lengths, key_lengths, q.device)
        if hidden is not None:   # the dead rows of q, k and v are zeros, whatever the inputs hold there
            q, kv = q.masked_fill(dead_q, 0.0), kv.masked_fill(dead_k, 0.0)
        qh, k, v = self.split(q, kv, d)
        s = (qh @ k.transpose(-1, -2)) * self.scale_for(d)                 # (the matmul broadcasts k and v over the group)
        if hidden is not None:
            s = s.masked_fill(hidden, float("-inf"))
        out = (s.softmax(-1) @ v).reshape(N, H, Tq, d).transpose(1, 2).reshape(N, Tq, H * d)
        return out if dead_q is None else out.masked_fill(dead_q, 0.0)     # (a dead query saw key 0, which may be live)


class MultiheadCrossAttention(nn.Module):
    """``nn.MultiheadAttention(batch_first=True)`` applied to ``(x, memory, memory)`` as a container of leaves the extensions have
    rules for: ``q_proj = Linear(E, H d)`` on ``x [N, Tq, E]``, ``kv_proj = Linear(kdim or E, 2 Hkv d)`` on ``memory [N, Tk, kdim]``,
    :class:`ScaledDotProductCrossAttention`, ``out_proj = Linear(E, E)``; ``d = E / H``, ``Hkv = num_kv_heads or H``.  ``set_lengths``
    is that of the leaf (right-padded batches on either side).  No causal mask, no window, no dropout, no arbitrary mask."""

    def __init__(self, embed_dim: int, num_heads: int, bias: bool = True, num_kv_heads: int = None, kdim: int = None):
        super().__init__()
        if embed_dim % num_heads != 0:
            raise ValueError(f"embed_dim ({embed_dim}) is not divisible by num_heads ({num_heads})")
        self.attention = ScaledDotProductCrossAttention(num_heads, num_kv_heads=num_kv_heads)
        self.embed_dim, self.num_heads, self.kdim = int(embed_dim), int(num_heads), int(embed_dim if kdim is None else kdim)
        self.q_proj = nn.Linear(embed_dim, embed_dim, bias=bias)
        self.kv_proj = nn.Linear(self.kdim, 2 * self.attention.kv_heads * (embed_dim // num_heads), bias=bias)
        self.out_proj = nn.Linear(embed_dim, embed_dim, bias=bias)

    def forward(self, x: Tensor, memory: Tensor) -> Tensor:
        return self.out_proj(self.attention(self.q_proj(x), self.kv_proj(memory)))

    def set_lengths(self, query_lengths=None, key_lengths=None) -> None:
        """Per-sample lengths of ``x`` and of ``memory`` for the padded batches to come (``None``: none), handed to the leaf."""
        self.attention.set_lengths(query_lengths, key_lengths)

    @classmethod
    def from_torch(cls, mha: nn.MultiheadAttention) -> "MultiheadCrossAttention":
        """A copy of ``mha``'s projections: of a packed ``in_proj_weight`` the rows ``[:E]`` go to ``q_proj`` and the rows ``[E:]`` (k | v)
        to ``kv_proj``; of separate ``q / k / v_proj_weight`` (``kdim != embed_dim``) k and v are stacked, which needs ``kdim == vdim``."""
        if mha.kdim != mha.vdim:
            raise ValueError("nn.MultiheadAttention with equal k / v dimensions is required")
        if not mha.batch_first or mha.bias_k is not None or mha.add_zero_attn or mha.dropout != 0.0:
            raise ValueError("batch_first=True, no dropout, no bias_k / bias_v and no add_zero_attn are required")
        E = mha.embed_dim
        if mha.in_proj_weight is not None:
            wq, wkv = mha.in_proj_weight[:E], mha.in_proj_weight[E:]
        else:
            wq, wkv = mha.q_proj_weight, torch.cat((mha.k_proj_weight, mha.v_proj_weight), 0)
        new = cls(E, mha.num_heads, bias=mha.in_proj_bias is not None, kdim=mha.kdim).to(device=wq.device, dtype=wq.dtype)
        with torch.no_grad():
            new.q_proj.weight.copy_(wq)
            new.kv_proj.weight.copy_(wkv)
            new.out_proj.weight.copy_(mha.out_proj.weight)
            if mha.in_proj_bias is not None:
                new.q_proj.bias.copy_(mha.in_proj_bias[:E])
                new.kv_proj.bias.copy_(mha.in_proj_bias[E:])
                new.out_proj.bias.copy_(mha.out_proj.bias)
        return new
