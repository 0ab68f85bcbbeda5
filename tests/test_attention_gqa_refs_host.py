"""Host checks of tests/attention_gqa_refs.py and of the torch restatements of the grouped-query rules (no GPU).  The reference agrees
with fp64 autograd of a forward pass this file writes on its own (``repeat_interleave``, then
``torch.nn.functional.scaled_dot_product_attention``) and, at ``Hkv == H``, with ``attention_refs.rule``; the rules the factor
provider uses for non-HIP tensors (``_attention_jac_t_torch``, ``_rope_jac_t_torch``), on modules built with ``num_kv_heads``, stay
inside the derived bounds in fp32, which makes the bounds a property of the reference and of fp32 arithmetic and not of the kernel
they judge."""
import pytest
import torch
import torch.nn.functional as F

import attention_gqa_refs as gr
import attention_refs as ar
from vivit_amd.backend import RotaryEmbedding, ScaledDotProductAttention
from vivit_amd.backend.extensions import _attention_jac_t_torch, _rope_jac_t_torch

_REFS = {}


def operands(case):
    """The operands of a case as tests/test_attention_gqa_rule_gpu.py makes them, with the fp64 reference (computed once)."""
    if case not in _REFS:
        T, d, H, Hkv, V, N, causal, scale = case
        M, qkv, out, scale = gr.make_case(1000 * T + d + H, V, N, T, H, Hkv, d, scale, causal)
        _REFS[case] = (M, qkv, out, scale) + gr.rule(M, qkv, out, H, Hkv, scale, causal)
    return _REFS[case]


def sdpa_forward(qkv, H, Hkv, scale, causal):
    """An independent forward pass: K and V copied to H heads, torch's own attention."""
    N, T, W = qkv.shape
    d, R = W // (H + 2 * Hkv), H // Hkv
    q = qkv[..., :H * d].view(N, T, H, d).transpose(1, 2)
    k = qkv[..., H * d:(H + Hkv) * d].view(N, T, Hkv, d).transpose(1, 2).repeat_interleave(R, 1)
    v = qkv[..., (H + Hkv) * d:].view(N, T, Hkv, d).transpose(1, 2).repeat_interleave(R, 1)
    return F.scaled_dot_product_attention(q, k, v, is_causal=causal, scale=scale).transpose(1, 2).reshape(N, T, H * d)


@pytest.mark.parametrize("case", [c for c in gr.CASES if c[0] <= 33 and c[7] != 0.0], ids=str)
def test_reference_is_the_transposed_jacobian_of_an_independent_forward(case):
    T, d, H, Hkv, V, N, causal, _ = case
    M, qkv, out, scale, ref, _ = operands(case)
    x = qkv.double().requires_grad_(True)
    y = sdpa_forward(x, H, Hkv, scale, causal)
    assert (y.detach() - gr.forward(qkv.double(), H, Hkv, scale, causal)).abs().max().item() <= 1e-12 * max(1.0, y.abs().max().item())
    # the reference takes the fp32 module output as an input: hand it the fp64 one for this comparison
    ref64, _ = gr.rule(M, qkv, y.detach(), H, Hkv, scale, causal)
    for vi in range(V):
        (g,) = torch.autograd.grad(y, x, M[vi].double(), retain_graph=True)
        assert (g - ref64[vi]).abs().max().item() <= 1e-11 * max(1.0, ref64[vi].abs().max().item())
    # and with the fp32 output it differs only through D: well inside the bound
    assert ((ref - ref64).abs() / gr.rule(M, qkv, out, H, Hkv, scale, causal)[1]).max().item() <= 1.0


@pytest.mark.parametrize("case", [c for c in ar.CASES if c[0] in (5, 33)][:6], ids=str)
def test_equal_head_counts_reproduce_the_multi_head_reference(case):
    T, d, H, V, N, causal, scale = case
    M, qkv, out, scale = ar.make_case(1000 * T + d, V, N, T, H, d, scale, causal)
    ref, bound = ar.rule(M, qkv, out, H, scale, causal)
    got, gbound = gr.rule(M, qkv, out, H, H, scale, causal)
    torch.testing.assert_close(got, ref, rtol=1e-12, atol=0.0)
    torch.testing.assert_close(gbound, bound, rtol=1e-12, atol=0.0)
    assert torch.equal(gr.forward(qkv, H, H, scale, causal), out)


def test_the_rule_of_the_case_list_holds():
    assert len(set(gr.CASES)) == len(gr.CASES) and 20 <= len(gr.CASES) <= 30
    for lo, hi in gr.INSTANCES:
        mine = [c for c in gr.CASES if lo <= c[1] <= hi]
        VC = gr.chunk(lo)
        assert gr.chunk(hi) == VC and lo % 4 != 0
        assert {lo, hi} <= {c[1] for c in mine}
        assert {2, 3, 4} <= {c[2] // c[3] for c in mine} and {1, 2, 3} <= {c[3] for c in mine}
        assert {VC - 1, VC, 2 * VC + 1} <= {c[4] for c in mine}
        assert {1, 5, 32, 33, 65} <= {c[0] for c in mine}
        assert {False, True} == {c[6] for c in mine} and {1, 2} == {c[5] for c in mine}
    assert all(c[2] % c[3] == 0 and c[3] < c[2] for c in gr.CASES)
    assert any(c[7] is not None and c[7] < 0 for c in gr.CASES) and any(c[7] == 0.0 for c in gr.CASES)
    assert all(c[0] <= 65 and c[2] <= 6 and c[1] <= 128 and c[4] <= 9 and c[5] <= 2 for c in gr.CASES)


@pytest.mark.parametrize("case", gr.CASES, ids=str)
def test_torch_rule_of_the_module_stays_within_the_bounds(case):
    """``_attention_jac_t_torch`` in fp32 on a module built with ``num_kv_heads``; the module's forward is the reference's."""
    T, d, H, Hkv, V, N, causal, _ = case
    M, qkv, out, scale, ref, bound = operands(case)
    assert ref.shape == bound.shape == (V, N, T, (H + 2 * Hkv) * d) and bool((bound > 0).all())
    module = ScaledDotProductAttention(H, causal=causal, scale=scale, num_kv_heads=Hkv)
    fwd = module(qkv)
    assert fwd.shape == out.shape and (fwd - out).abs().max().item() <= 1e-5 * max(1.0, out.abs().max().item())
    got = _attention_jac_t_torch(module, M, qkv, out)
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    ratio = ((got.double() - ref).abs() / bound).max().item()
    print(f"max error / bound = {ratio:.3g}")
    assert ratio <= 0.5, ratio


def test_torch_rule_with_large_logits_stays_within_the_bounds():
    V, N, T, H, Hkv, d = 3, 2, 33, 4, 2, 20
    M, qkv, out, scale = gr.make_case(7, V, N, T, H, Hkv, d, None, True, qk_gain=8.0)
    S = gr.logits(qkv, H, Hkv, scale)
    assert S.max().item() > 150 and S.min().item() < -150
    ref, bound = gr.rule(M, qkv, out, H, Hkv, scale, True)
    got = _attention_jac_t_torch(ScaledDotProductAttention(H, causal=True, num_kv_heads=Hkv), M, qkv, out)
    assert ((got.double() - ref).abs() / bound).max().item() <= 0.5


def test_a_wrong_group_falls_outside_the_bounds():
    """The mistake the layout invites: heads dealt to the groups round-robin (h % Hkv) and not in consecutive runs (h // R)."""
    V, N, T, H, Hkv, d = 3, 1, 33, 4, 2, 20
    M, qkv, out, scale = gr.make_case(5, V, N, T, H, Hkv, d, None, True)
    ref, bound = gr.rule(M, qkv, out, H, Hkv, scale, True)
    swap = [0, 2, 1, 3]                                                   # query heads permuted so that h % Hkv becomes h // R
    perm_q = qkv.clone()
    perm_q[..., :H * d] = qkv[..., :H * d].view(N, T, H, d)[:, :, swap].reshape(N, T, H * d)
    pm = M.view(V, N, T, H, d)[:, :, :, swap].reshape(V, N, T, H * d)
    po = out.view(N, T, H, d)[:, :, swap].reshape(N, T, H * d)
    wrong = _attention_jac_t_torch(ScaledDotProductAttention(H, causal=True, num_kv_heads=Hkv), pm, perm_q, po)
    assert not gr.within(wrong[..., H * d:], ref[..., H * d:], bound[..., H * d:])[0]


@pytest.mark.parametrize("T", gr.ROPE_T)
@pytest.mark.parametrize("d", gr.ROPE_D)
@pytest.mark.parametrize("H,Hkv", gr.ROPE_HEADS)
def test_torch_rotary_rule_stays_within_the_bound(H, Hkv, d, T):
    g = gr.gen(d + 10 * T + H + Hkv)
    V, N = 2, 3
    M = gr.lr.generic(g, V, N, T, (H + 2 * Hkv) * d)
    module = RotaryEmbedding(H, num_kv_heads=Hkv)
    x = torch.zeros(N, T, (H + 2 * Hkv) * d)
    cos, sin = module.tables(T, d, x.device, x.dtype)
    ref, bound = gr.rope(M.view(V * N, T, -1), cos, sin, H, Hkv)
    got = _rope_jac_t_torch(module, M, x)
    assert got.shape == M.shape
    ok, msg = gr.within(got.view(V * N, T, -1), ref, bound)
    assert ok, msg
    assert torch.equal(got[..., (H + Hkv) * d:], M[..., (H + Hkv) * d:])   # v: bit for bit
    if Hkv == H:                                                          # the layout of three equal thirds: the old formula's bytes
        assert torch.equal(got, _rope_jac_t_torch(RotaryEmbedding(H), M, x))
    # the rule inverts the module's forward pass (a rotation's transpose is its inverse)
    xin = gr.lr.generic(g, N, T, (H + 2 * Hkv) * d)
    back = _rope_jac_t_torch(module, module(xin)[None], xin)[0]
    assert (back.double() - xin.double()).abs().max().item() <= 14 * gr.EPS * 2 * xin.abs().max().item()
