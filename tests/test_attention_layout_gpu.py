"""One head layout from module to kernel, on the device.  ``kernels.attention_jac_t`` and ``kernels.rope_jac_t`` without
``num_kv_heads`` go through ``vivit_attention_masked_jac_t_f32`` and ``vivit_rope_gqa_jac_t_f32`` with ``Hkv = H``: their results must be
the bytes of a direct call of the legacy entries ``vivit_attention_jac_t_f32`` (on a workspace of its own, sized by its own query)
and ``vivit_rope_jac_t_f32`` on the same operands.  The fp32 forward passes of the modules and their gradients must be the bytes of
the frozen multi-head formulas of tests/test_attention_layout_host.py.

Shapes: V = 3 and 5 factor rows (a partial chunk and more than one chunk of 4), T = 33 (two key blocks, the second ragged), d = 5
(scalar loads) and 16 (16-byte loads); the rotary rule with d = 4 (scalar body) and 8 (16-byte body)."""
import pytest
import torch

from test_attention_layout_host import frozen_attend, frozen_rope, grad_of
from vivit_amd import _lib, kernels
from vivit_amd.backend import RotaryEmbedding, ScaledDotProductAttention

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("d", (5, 16))
@pytest.mark.parametrize("V", (3, 5))
def test_attention_wrapper_is_the_legacy_entry(V, d, causal):
    N, T, H = 2, 33, 2
    g = torch.Generator().manual_seed(100 * V + d)
    qkv = torch.randn(N, T, 3 * H * d, generator=g).to(DEV)
    M = torch.randn(V, N, T, H * d, generator=g).to(DEV)
    scale = d ** -0.5
    out = ScaledDotProductAttention(H, causal=causal)(qkv).contiguous()
    got = kernels.attention_jac_t(M, qkv, out, H, scale, causal)

    lib = _lib.load()
    nbytes = lib.vivit_attention_jac_t_f32_workspace_bytes(V, N, T, H, d)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    want = torch.full((V, N, T, 3 * H * d), float("nan"), device=DEV)
    st = lib.vivit_attention_jac_t_f32(M.data_ptr(), qkv.data_ptr(), out.data_ptr(), want.data_ptr(), V, N, T, H, d, scale, int(causal),
                                       ws.data_ptr(), ws.numel(), stream())
    assert st == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want).all()) and torch.equal(got, want)


@pytest.mark.parametrize("d", (4, 8))
def test_rope_wrapper_is_the_legacy_entry(d):
    V, N, T, H = 2, 2, 5, 2
    g = torch.Generator().manual_seed(d)
    M = torch.randn(V, N, T, 3 * H * d, generator=g).to(DEV)
    cos, sin = RotaryEmbedding(H).tables(T, d, DEV, torch.float32)
    want = torch.full_like(M, float("nan"))
    st = _lib.load().vivit_rope_jac_t_f32(M.data_ptr(), cos.data_ptr(), sin.data_ptr(), want.data_ptr(), V * N, T, H, d, stream())
    assert st == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want).all())
    assert torch.equal(kernels.rope_jac_t(M, cos, sin, H), want)
    work = M.clone()
    assert kernels.rope_jac_t(work, cos, sin, H, out=work) is work and torch.equal(work, want)   # in place


@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
def test_attention_forward_is_the_frozen_multi_head_formula(causal):
    N, T, H, d = 2, 33, 3, 8
    g = torch.Generator().manual_seed(7)
    x, W = torch.randn(N, T, 3 * H * d, generator=g).to(DEV), torch.randn(N, T, H * d, generator=g).to(DEV)
    module, frozen = ScaledDotProductAttention(H, causal=causal), lambda t: frozen_attend(t, H, causal)   # noqa: E731
    assert torch.equal(module(x), frozen(x))
    assert torch.equal(grad_of(module, x, W), grad_of(frozen, x, W))


def test_rotary_forward_is_the_frozen_multi_head_formula():
    N, T, H, d = 2, 33, 3, 8
    g = torch.Generator().manual_seed(8)
    x, W = torch.randn(N, T, 3 * H * d, generator=g).to(DEV), torch.randn(N, T, 3 * H * d, generator=g).to(DEV)
    module, frozen = RotaryEmbedding(H), lambda t: frozen_rope(t, H)   # noqa: E731
    assert torch.equal(module(x), frozen(x))
    assert torch.equal(grad_of(module, x, W), grad_of(frozen, x, W))
