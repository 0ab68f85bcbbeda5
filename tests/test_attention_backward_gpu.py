"""``kernels.attention_backward`` and ``kernels.cross_attention_backward`` (csrc/attention_backward.hip) on the device's own forward
pass (``out`` and ``lse`` of ``return_lse=True``) against the fp64 rule with one factor row under its derived bounds
(``sr.rule(M[:1], ...)``, ``cr.rule(M[:1], ...)``), on the cases of the rule's own tests and three plain self-attention cases, and what
the kernels promise: exact zeros at dead rows; the same bytes from a second call; per padded sample the bytes of the sample cut to its
length -- every operand -- and run alone; NaN and inf at dead positions of every operand change no byte; either cross result alone
has the bytes of the full call; operands four bytes off a 16-byte boundary; the module with ``fused_forward=True`` reaches the kernel.

On the commit before the feature every test of this file fails: the launchers do not exist."""
import pytest
import torch

import attention_cross_refs as cr
import attention_forward_refs as fr
import attention_scoremod_refs as sr
from vivit_amd import kernels
from vivit_amd.backend import ScaledDotProductAttention

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLAIN = [(33, 16, 2, 2, False, None, None), (97, 64, 4, 1, True, (97, 40, 0), 33), (161, 128, 6, 3, False, (161, 64), None)]


def dev(t):
    return None if t is None else t.to(DEV)


def check(name, got, ref, bound):
    """Finite, within the bound, exact zeros at the dead rows (whose bound is 2^-126)."""
    got = got.cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    print(f"{name}: max error / bound = {((got.double() - ref).abs() / bound).max().item():.3g}")
    ok, msg = fr.within(got, ref, bound)
    assert ok, (name, msg)
    assert bool((got[bound == fr.FLT_MIN] == 0).all())


def poison(t, dead_rows):
    """``t [N, T, C]`` on the device with NaN and inf in its dead rows."""
    t = t.clone()
    t[dev(dead_rows)] = float("nan")
    t[..., ::2][dev(dead_rows)] = float("inf")
    return t


def self_checks(M, qkv, H, Hkv, He, scale, causal, lengths, window, cap, table):
    N, T, _ = qkv.shape
    kw = dict(num_kv_heads=Hkv, lengths=lengths, window=window, softcap=cap, bias=dev(table))
    dout, x = dev(M[0]), dev(qkv)
    out, lse = kernels.attention_forward(x, H, scale, causal, return_lse=True, **kw)
    got = kernels.attention_backward(dout, x, out, lse, H, scale, causal, **kw)
    check("dqkv", got, *(r[0] for r in sr.rule(M[:1], qkv, out.cpu(), H, He, scale, causal, lengths, window, cap, table)))
    assert torch.equal(kernels.attention_backward(dout, x, out, lse, H, scale, causal, **kw), got)
    if lengths is None:
        return
    for n, L in enumerate(lengths):
        assert bool((got[n, L:] == 0).all()), n
        if L > 0:
            cut = dict(kw, lengths=None, bias=None if table is None else dev(table[:, T - L:T + L - 1].contiguous()))
            alone = kernels.attention_backward(*(t[n:n + 1, :L].contiguous() for t in (dout, x, out)), lse[n:n + 1, :, :L].contiguous(),
                                               H, scale, causal, **cut)
            assert torch.equal(got[n, :L], alone[0]), (n, L)
    dd = sr.dead(T, lengths, N)
    lse2 = poison(lse.transpose(1, 2), dd).transpose(1, 2).contiguous()
    assert torch.equal(kernels.attention_backward(poison(dout, dd), poison(x, dd), poison(out, dd), lse2, H, scale, causal, **kw), got)


@pytest.mark.parametrize("i", range(len(sr.CASES)))
def test_self_attention_cases(i):
    T, d, H, Hkv, _, N, causal, _, lengths, window, cap, _ = sr.CASES[i]
    M, qkv, _, scale, He, table = sr.case_operands(sr.CASES[i])
    self_checks(M, qkv, H, Hkv, He, scale, causal, lengths, window, cap, table)


@pytest.mark.parametrize("T,d,H,Hkv,causal,lengths,window", PLAIN)
def test_plain_self_attention_cases(T, d, H, Hkv, causal, lengths, window):
    """No cap and no table: the ``AttPlain`` instances of the self-attention geometry."""
    M, qkv, _, scale = sr.make_case(T + d, 1, 2 if lengths is None else len(lengths), T, H, Hkv, d, None, causal, lengths, window)
    self_checks(M, qkv, H, Hkv, Hkv, scale, causal, lengths, window, None, None)


@pytest.mark.parametrize("i", range(len(cr.CASES)))
def test_cross_attention_cases(i):
    Tq, Tk, d, H, Hkv, _, N, _, ql, kl = cr.CASES[i]
    M, q, kv, _, scale, He = cr.case_operands(cr.CASES[i])
    kw = dict(num_kv_heads=Hkv, query_lengths=ql, key_lengths=kl)
    dout, a, b = dev(M[0]), dev(q), dev(kv)
    out, lse = kernels.cross_attention_forward(a, b, H, scale, return_lse=True, **kw)
    dq, dkv = kernels.cross_attention_backward(dout, a, b, out, lse, H, scale, **kw)
    Gq, e_q, Gkv, e_kv = cr.rule(M[:1], q, kv, out.cpu(), H, He, scale, ql, kl)
    check("dq", dq, Gq[0], e_q[0])
    check("dkv", dkv, Gkv[0], e_kv[0])
    again = kernels.cross_attention_backward(dout, a, b, out, lse, H, scale, **kw)
    assert torch.equal(again[0], dq) and torch.equal(again[1], dkv)
    only_q = kernels.cross_attention_backward(dout, a, b, out, lse, H, scale, want=(True, False), **kw)
    only_kv = kernels.cross_attention_backward(dout, a, b, out, lse, H, scale, want=(False, True), **kw)
    assert only_q[1] is None and torch.equal(only_q[0], dq) and only_kv[0] is None and torch.equal(only_kv[1], dkv)
    if ql is None and kl is None:
        return
    for n, (Lq, Lk) in enumerate(cr.live_lengths(Tq, Tk, ql, kl, N)):
        assert bool((dq[n, Lq:] == 0).all()) and bool((dkv[n, Lk:] == 0).all()), n
        if Lq > 0:
            alone = kernels.cross_attention_backward(dout[n:n + 1, :Lq].contiguous(), a[n:n + 1, :Lq].contiguous(), b[n:n + 1, :Lk].contiguous(),
                                                     out[n:n + 1, :Lq].contiguous(), lse[n:n + 1, :, :Lq].contiguous(), H, scale,
                                                     num_kv_heads=Hkv)
            assert torch.equal(dq[n, :Lq], alone[0][0]) and torch.equal(dkv[n, :Lk], alone[1][0]), (n, Lq, Lk)
    deadq, deadk = cr.dead(Tq, Tk, ql, kl, N)
    lse2 = poison(lse.transpose(1, 2), deadq).transpose(1, 2).contiguous()
    got = kernels.cross_attention_backward(poison(dout, deadq), poison(a, deadq), poison(b, deadk), poison(out, deadq), lse2, H, scale, **kw)
    assert torch.equal(got[0], dq) and torch.equal(got[1], dkv)


@pytest.mark.parametrize("which", ["dout", "qkv", "out", "q", "kv"])
def test_operand_four_bytes_off_a_16_byte_boundary(which):
    if which in ("dout", "qkv", "out"):
        T, d, H, Hkv, lengths = 40, 64, 4, 2, (40, 31)
        table = dev(sr.make_table("normal", 5, H, T))
        M, qkv, _, scale = sr.make_case(21, 1, 2, T, H, Hkv, d, None, True, lengths, 33)
        kw = dict(num_kv_heads=Hkv, lengths=lengths, window=33, softcap=2.0, bias=table)
        ops = {"dout": dev(M[0]), "qkv": dev(qkv)}
        ops["out"], lse = kernels.attention_forward(ops["qkv"], H, scale, True, return_lse=True, **kw)
        call = lambda: (kernels.attention_backward(ops["dout"], ops["qkv"], ops["out"], lse, H, scale, True, **kw),)   # noqa: E731
    else:
        M, q, kv, _, scale = cr.make_case(22, 1, 2, 40, 70, 4, 2, 64, None, (40, 31), (70, 33))
        kw = dict(num_kv_heads=2, query_lengths=(40, 31), key_lengths=(70, 33))
        ops = {"dout": dev(M[0]), "q": dev(q), "kv": dev(kv)}
        ops["out"], lse = kernels.cross_attention_forward(ops["q"], ops["kv"], 4, scale, return_lse=True, **kw)
        call = lambda: kernels.cross_attention_backward(ops["dout"], ops["q"], ops["kv"], ops["out"], lse, 4, scale, **kw)   # noqa: E731
    aligned = call()
    ops[which] = sr.misaligned(ops[which])
    assert all(torch.equal(g, a) for g, a in zip(call(), aligned))


def test_the_module_reaches_the_kernel():
    """GQA, causal, lengths: ``x.grad`` of the module has the bytes of the launcher on the same operands."""
    T, d, H, Hkv, lengths = 70, 20, 4, 2, (70, 33, 0)
    g = sr.gen(3)
    x, W = dev(torch.randn(3, T, (H + 2 * Hkv) * d, generator=g)).requires_grad_(), dev(torch.randn(3, T, H * d, generator=g))
    module = ScaledDotProductAttention(H, causal=True, num_kv_heads=Hkv, fused_forward=True)
    module.set_lengths(lengths)
    (module(x) * W).sum().backward()
    out, lse = kernels.attention_forward(x.detach(), H, d ** -0.5, True, num_kv_heads=Hkv, lengths=lengths, return_lse=True)
    ref = kernels.attention_backward(W, x.detach(), out, lse, H, d ** -0.5, True, num_kv_heads=Hkv, lengths=lengths)
    assert float(ref.abs().max()) > 0 and torch.equal(x.grad, ref)
