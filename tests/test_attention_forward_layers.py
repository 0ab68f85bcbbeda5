"""The attention modules with ``fused_forward=True`` on the device: output, input gradients and the learned table's gradient from
``loss.backward()`` against fp64 autograd of the torch formula -- the output under the bound of tests/attention_forward_refs.py, the
gradients under the rule's own bounds with V = 1 (the gradient at the output is the one factor row) --, a frozen memory skips its
owner, and ``SqrtGGNExact`` on a small model agrees with and without the flag.

On the commit before the feature every test of this file fails: the modules take no ``fused_forward``."""
import pytest
import torch
from torch import nn

import attention_bias_refs as br
import attention_cross_refs as cr
import attention_forward_refs as fr
import attention_scoremod_refs as sr
from vivit_amd.backend import (MultiheadSelfAttention, ScaledDotProductAttention, ScaledDotProductCrossAttention, SqrtGGNExact, backpack,
                               extend)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def close(name, got, ref, bound):
    print(f"{name}: max error / bound = {((got.cpu().double() - ref).abs() / bound).max().item():.3g}")
    ok, msg = fr.within(got.cpu(), ref, bound)
    assert ok, (name, msg)


@pytest.mark.parametrize("T,d,H,Hkv,lengths,cap", [(33, 20, 4, 2, (33, 17, 0), 1.5), (97, 64, 4, 1, (97, 40), 2.0)])
def test_self_attention_module(T, d, H, Hkv, lengths, cap):
    """GQA, a causal mask, lengths, a cap and a learned table built for three positions more than the batch has."""
    g = sr.gen(T + d)
    N, scale = len(lengths), d ** -0.5
    param = torch.randn(H, 2 * (T + 3) - 1, generator=g)
    qkv, W = torch.randn(N, T, (H + 2 * Hkv) * d, generator=g), torch.randn(N, T, H * d, generator=g)
    results = []
    for device, dtype, fused in ((DEV, torch.float32, True), ("cpu", sr.F64, False)):
        module = ScaledDotProductAttention(H, causal=True, num_kv_heads=Hkv, softcap=cap, bias=param, learn_bias=True,
                                           fused_forward=fused).to(device=device, dtype=dtype)
        module.set_lengths(lengths)
        x = qkv.to(device=device, dtype=dtype).requires_grad_()
        out = module(x)
        (out * W.to(device=device, dtype=dtype)).sum().backward()
        results.append((out.detach(), x.grad, module.bias.grad))
    (out, dx, db), (out64, dx64, db64) = results
    table, index = param[:, 3:-3].contiguous(), torch.arange(3, 2 * T + 2)   # the middle slice, and where it sits in the parameter
    close("out", out, out64, fr.self_forward(qkv, H, Hkv, scale, True, lengths, None, cap, table)[1])
    operands = (W[None], qkv, out.cpu(), H, Hkv, scale, True, lengths, None, cap, table)
    close("qkv.grad", dx, dx64, sr.rule(*operands)[1][0])
    Gb, e_Gb = br.factor(*operands, index, param.shape[1])
    close("bias.grad", db, db64, (e_Gb[0] + (N + 2) * sr.EPS * Gb[0].abs()).sum(0))   # (and the sum over the N samples)
    assert float(db64.abs().max()) > 1e-3 and bool((dx[sr.dead(T, lengths, N)] == 0).all())


@pytest.mark.parametrize("Tq,Tk,d,H,Hkv,ql,kl", [(33, 97, 20, 4, 2, (33, 17, 5), (97, 40, 0)), (97, 33, 64, 4, 1, (97, 40), (32, 33))])
def test_cross_attention_module(Tq, Tk, d, H, Hkv, ql, kl):
    g = sr.gen(Tq + d)
    N, scale = len(ql), d ** -0.5
    q, kv, W = torch.randn(N, Tq, H * d, generator=g), torch.randn(N, Tk, 2 * Hkv * d, generator=g), torch.randn(N, Tq, H * d, generator=g)
    results = []
    for device, dtype, fused, frozen in ((DEV, torch.float32, True, False), ("cpu", sr.F64, False, False), (DEV, torch.float32, True, True)):
        module = ScaledDotProductCrossAttention(H, num_kv_heads=Hkv, fused_forward=fused)
        module.set_lengths(ql, kl)
        a, b = q.to(device=device, dtype=dtype).requires_grad_(), kv.to(device=device, dtype=dtype).requires_grad_(not frozen)
        out = module(a, b)
        (out * W.to(device=device, dtype=dtype)).sum().backward()
        results.append((out.detach(), a.grad, b.grad))
    (out, dq, dkv), (out64, dq64, dkv64), (_, dq_frozen, none) = results
    close("out", out, out64, fr.cross_forward(q, kv, H, Hkv, scale, ql, kl)[1])
    _, e_q, _, e_kv = cr.rule(W[None], q, kv, out.cpu(), H, Hkv, scale, ql, kl)
    close("q.grad", dq, dq64, e_q[0])
    close("kv.grad", dkv, dkv64, e_kv[0])
    assert none is None and torch.equal(dq_frozen, dq)


def test_sqrt_ggn_exact_agrees_with_and_without_the_flag():
    """Both runs are the fp32 device path of tests/test_attention_scoremod_layers.py, which holds each within rtol 1e-4, atol 1e-6 of
    the fp64 oracle: they agree with each other within twice that."""
    E, H, T, N, C = 16, 4, 33, 3, 3
    g = sr.gen(5)
    X, y = torch.randn(N, T, E, generator=g).to(DEV), torch.randint(0, C, (N,), generator=g).to(DEV)
    factors = []
    for fused in (False, True):
        torch.manual_seed(0)
        attention = MultiheadSelfAttention(E, H, causal=True, num_kv_heads=2, softcap=2.0, fused_forward=fused)
        attention.set_lengths([33, 20, 1])
        model = extend(nn.Sequential(attention, nn.Flatten(), nn.Linear(T * E, C)).to(DEV))
        loss = extend(nn.CrossEntropyLoss())(model(X), y)
        with backpack(SqrtGGNExact()):
            loss.backward()
        factors.append([p.sqrt_ggn_exact for p in model.parameters()])
    for a, b in zip(*factors):
        assert float(a.abs().max()) > 0
        torch.testing.assert_close(b, a, rtol=2e-4, atol=2e-6)
