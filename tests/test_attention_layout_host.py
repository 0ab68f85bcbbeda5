"""One head layout from module to kernel: the attention and rotary modules and their torch rules treat ``num_kv_heads=None`` as
``Hkv = H`` and compute with the grouped formulas alone.  The multi-head formulas they had before -- the ``view(N, T, 3, H, d)``
forward pass and rule, the ``view(N, T, 3, H, d)`` rotation and its transpose -- are frozen in this file, and what the modules
compute without ``num_kv_heads`` must be their bytes (``torch.equal``, no tolerance): the forward pass, the torch rules and the
gradient of each forward pass with respect to its input.  ``Module(H)`` and ``Module(H, num_kv_heads=H)`` must agree bytewise on
all of it, and ``num_kv_heads`` stays ``None`` on a module built without it."""
import pytest
import torch

from vivit_amd.backend import MultiheadSelfAttention, RotaryEmbedding, ScaledDotProductAttention
from vivit_amd.backend.extensions import _attention_jac_t_torch, _rope_jac_t_torch

SHAPES = ((2, 5, 3, 4), (3, 33, 2, 16), (2, 65, 4, 6), (1, 1, 1, 2), (2, 97, 6, 34), (4, 128, 8, 64))   # (N, T, H, d)
MASKS = ("none", "window", "lengths", "zero_lengths")
V = 3


# ---- the multi-head formulas of the commit before the fold, frozen ----

def frozen_hidden(T, lengths, causal, window, device):
    """The pairs that do not see each other, ``[T, T]``, ``[N | 1, T, T]`` or ``None``."""
    if lengths is None and window is None:
        return torch.ones(T, T, dtype=torch.bool, device=device).triu(1) if causal else None
    t = torch.arange(T, device=device)
    dist = t[:, None] - t[None, :]
    vis = torch.ones(1, T, T, dtype=torch.bool, device=device)
    if causal:
        vis = vis & (dist >= 0)
    if window is not None:
        vis = vis & (dist.abs() < window)
    if lengths is not None:
        live = t[None, :] < lengths[:, None]
        vis = (vis & live[:, :, None] & live[:, None, :]) | (dist == 0)
    return ~vis


def frozen_dead(T, lengths, device):
    return (torch.arange(T, device=device)[None, :] >= lengths[:, None])[:, :, None]


def frozen_attend(qkv, H, causal, lengths=None, window=None):
    N, T, d = qkv.shape[0], qkv.shape[1], qkv.shape[2] // (3 * H)
    hidden = frozen_hidden(T, lengths, causal, window, qkv.device)
    if lengths is not None:
        qkv = qkv.masked_fill(frozen_dead(T, lengths, qkv.device), 0.0)
    q, k, v = qkv.view(N, T, 3, H, d).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * d ** -0.5
    if hidden is not None:
        s = s.masked_fill(hidden if hidden.dim() == 2 else hidden[:, None], float("-inf"))
    return (s.softmax(-1) @ v).transpose(1, 2).reshape(N, T, H * d)


def frozen_attention_jac_t(M, x, out, H, causal, lengths=None, window=None):
    Vn, (N, T), d = M.shape[0], x.shape[:2], x.shape[2] // (3 * H)
    scale = d ** -0.5
    hidden = frozen_hidden(T, lengths, causal, window, x.device)
    if lengths is not None:
        dead = frozen_dead(T, lengths, x.device)
        M, x, out = M.reshape(Vn, N, T, -1).masked_fill(dead, 0.0), x.masked_fill(dead, 0.0), out.masked_fill(dead, 0.0)
    q, k, v = x.view(N, T, 3, H, d).permute(2, 0, 3, 1, 4)
    S = (q @ k.transpose(-1, -2)) * scale
    if hidden is not None:
        S = S.masked_fill(hidden if hidden.dim() == 2 else hidden[:, None], float("-inf"))
    P = S.softmax(-1)
    dO = M.reshape(Vn, N, T, H, d).permute(0, 1, 3, 2, 4)
    D = (dO * out.view(N, T, H, d).permute(0, 2, 1, 3)).sum(-1, keepdim=True)
    dV = P.transpose(-1, -2) @ dO
    dS = P * (dO @ v.transpose(-1, -2) - D)
    dQ, dK = (dS @ k) * scale, (dS.transpose(-1, -2) @ q) * scale
    G = torch.stack((dQ, dK, dV), 0).permute(1, 2, 4, 0, 3, 5).reshape(Vn, N, T, 3 * H * d)
    return G if lengths is None else G.masked_fill(dead, 0.0)


def frozen_tables(T, d, device, dtype, base=10000.0):
    j = torch.arange(d // 2, dtype=torch.float32, device=device)
    angle = torch.arange(T, dtype=torch.float32, device=device)[:, None] * (base ** (-2.0 * j / d))[None, :]
    return angle.cos().to(dtype), angle.sin().to(dtype)


def frozen_rope(qkv, H):
    N, T, d = qkv.shape[0], qkv.shape[1], qkv.shape[2] // (3 * H)
    half = d // 2
    cos, sin = (t.view(1, T, 1, 1, half) for t in frozen_tables(T, d, qkv.device, qkv.dtype))
    x = qkv.view(N, T, 3, H, d)
    x1, x2 = x[:, :, :2, :, :half], x[:, :, :2, :, half:]
    rot = torch.cat((x1 * cos - x2 * sin, x2 * cos + x1 * sin), -1)
    return torch.cat((rot, x[:, :, 2:]), 2).reshape(N, T, 3 * H * d)


def frozen_rope_jac_t(M, x, H):
    Vn, (N, T), d = M.shape[0], x.shape[:2], x.shape[2] // (3 * H)
    half = d // 2
    cos, sin = (t.view(1, 1, T, 1, 1, half) for t in frozen_tables(T, d, x.device, x.dtype))
    m = M.reshape(Vn, N, T, 3, H, d)
    m1, m2 = m[:, :, :, :2, :, :half], m[:, :, :, :2, :, half:]
    rot = torch.cat((m1 * cos + m2 * sin, m2 * cos - m1 * sin), -1)
    return torch.cat((rot, m[:, :, :, 2:]), 3).reshape(Vn, N, T, 3 * H * d)


# ---- the comparison ----

def mask_of(kind, N, T):
    """``(lengths, window)`` of a mask of the grid."""
    if kind == "window":
        return None, max(1, T // 3)
    if kind == "lengths":
        return [(3 * n + 1) * T // (3 * N) for n in range(N)], None   # distinct, from a short sample to nearly T
    if kind == "zero_lengths":
        return [0] * N, None
    return None, None


def grad_of(forward, x, W):
    x = x.clone().requires_grad_(True)
    return torch.autograd.grad((forward(x) * W).sum(), x)[0]


def operands(N, T, H, d, dtype):
    g = torch.Generator().manual_seed(1000 * T + 10 * H + d)
    draw = lambda *shape: torch.randn(*shape, generator=g, dtype=dtype)   # noqa: E731
    return draw(N, T, 3 * H * d), draw(V, N, T, H * d), draw(N, T, H * d), draw(V, N, T, 3 * H * d), draw(N, T, 3 * H * d)


@pytest.mark.parametrize("dtype", (torch.float32, torch.float64), ids=("fp32", "fp64"))
@pytest.mark.parametrize("N,T,H,d", SHAPES)
def test_attention_without_kv_heads_is_the_frozen_multi_head_formula(N, T, H, d, dtype):
    x, M, W, _, _ = operands(N, T, H, d, dtype)
    for causal in (False, True):
        for kind in MASKS:
            lengths, window = mask_of(kind, N, T)
            plain, same = (ScaledDotProductAttention(H, causal=causal, window=window, **kw) for kw in ({}, {"num_kv_heads": H}))
            assert plain.num_kv_heads is None and plain.kv_heads == H and same.num_kv_heads == H and same.kv_heads == H
            lt = None if lengths is None else torch.tensor(lengths, dtype=torch.int32)
            frozen = lambda t: frozen_attend(t, H, causal, lt, window)   # noqa: E731
            want_out = frozen(x)
            want_rule = frozen_attention_jac_t(M, x, want_out, H, causal, lt, window)
            want_grad = grad_of(frozen, x, W)
            for module in (plain, same):
                module.set_lengths(lengths)
                where = f"causal={causal} {kind} num_kv_heads={module.num_kv_heads}"
                out = module(x)
                assert torch.equal(out, want_out), where
                assert torch.equal(_attention_jac_t_torch(module, M, x, out, module.forward_lengths), want_rule), where
                assert torch.equal(grad_of(module, x, W), want_grad), where


@pytest.mark.parametrize("dtype", (torch.float32, torch.float64), ids=("fp32", "fp64"))
@pytest.mark.parametrize("N,T,H,d", SHAPES)
def test_rotary_without_kv_heads_is_the_frozen_multi_head_formula(N, T, H, d, dtype):
    x, _, _, M, W = operands(N, T, H, d, dtype)
    frozen = lambda t: frozen_rope(t, H)   # noqa: E731
    want_out, want_rule, want_grad = frozen(x), frozen_rope_jac_t(M, x, H), grad_of(frozen, x, W)
    plain, same = RotaryEmbedding(H), RotaryEmbedding(H, num_kv_heads=H)
    assert plain.num_kv_heads is None and plain.kv_heads == H and same.num_kv_heads == H and same.kv_heads == H
    for module in (plain, same):
        assert torch.equal(module(x), want_out)
        assert torch.equal(_rope_jac_t_torch(module, M, x), want_rule)
        assert torch.equal(grad_of(module, x, W), want_grad)


def test_num_kv_heads_stays_none_and_the_packed_width_follows_kv_heads():
    block = MultiheadSelfAttention(12, 6)
    assert block[1].num_kv_heads is None and block[1].kv_heads == 6 and block[0].out_features == 36
    grouped = MultiheadSelfAttention(12, 6, num_kv_heads=2)
    assert grouped[1].num_kv_heads == 2 and grouped[1].kv_heads == 2 and grouped[0].out_features == (6 + 2 * 2) * 2
    for module in (ScaledDotProductAttention(4), RotaryEmbedding(4)):
        with pytest.raises(AttributeError):
            module.kv_heads = 2
