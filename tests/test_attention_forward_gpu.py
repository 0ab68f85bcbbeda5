"""``kernels.attention_forward`` and ``kernels.cross_attention_forward`` (csrc/attention_forward.hip) against the fp64 reference under
the derived bounds of tests/attention_forward_refs.py, on the cases of the rule's own tests, and what the kernel promises: exact
zeros at dead rows; per padded sample the bytes of the sample cut to its length and run alone (with the table's middle slice); NaN
and inf at dead positions change no byte; ``return_lse`` changes no byte of ``out``; operands four bytes off a 16-byte boundary; no
``T x T`` allocation in forward + backward of a module with ``fused_forward=True``, where the torch formula makes several."""
import pytest
import torch

import attention_cross_refs as cr
import attention_forward_refs as fr
import attention_scoremod_refs as sr
from vivit_amd import kernels
from vivit_amd.backend import ScaledDotProductAttention

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def run_self(qkv, H, Hkv, scale, causal, lengths, window, cap, table, **kw):
    return kernels.attention_forward(qkv.to(DEV), H, scale, causal, num_kv_heads=Hkv, lengths=lengths, window=window, softcap=cap,
                                     bias=None if table is None else table.to(DEV), **kw)


def run_cross(q, kv, H, Hkv, scale, ql, kl, **kw):
    return kernels.cross_attention_forward(q.to(DEV), kv.to(DEV), H, scale, num_kv_heads=Hkv, query_lengths=ql, key_lengths=kl, **kw)


def check(got, lse, ref):
    """``out`` and ``lse`` within their bounds, finite, exact zeros at the dead rows (whose bound is 2^-126)."""
    out, e_out, ref_lse, e_lse = ref
    for name, g, r, b in (("out", got.cpu(), out, e_out), ("lse", lse.cpu(), ref_lse, e_lse)):
        assert g.shape == r.shape and bool(torch.isfinite(g).all())
        print(f"{name}: max error / bound = {((g.double() - r).abs() / b).max().item():.3g}")
        ok, msg = fr.within(g, r, b)
        assert ok, (name, msg)
        assert bool((g[b == fr.FLT_MIN] == 0).all())


@pytest.mark.parametrize("i", range(len(sr.CASES)))
def test_self_attention_cases(i):
    T, d, H, Hkv, _, N, causal, _, lengths, window, cap, _ = sr.CASES[i]
    _, qkv, _, scale, He, table = sr.case_operands(sr.CASES[i])
    args = (H, Hkv, scale, causal, lengths, window, cap, table)
    got, lse = run_self(qkv, *args, return_lse=True)
    check(got, lse, fr.self_forward(qkv, H, He, scale, causal, lengths, window, cap, table))
    assert torch.equal(run_self(qkv, *args), got)
    if lengths is None:
        return
    for n, L in enumerate(lengths):
        assert bool((got[n, L:] == 0).all()) and bool((lse[n, :, L:] == 0).all()), n
        if L > 0:
            middle = None if table is None else table[:, T - L:T + L - 1].contiguous()
            alone = run_self(qkv[n:n + 1, :L].contiguous(), H, Hkv, scale, causal, None, window, cap, middle)
            assert torch.equal(got[n, :L], alone[0]), (n, L)
    poisoned = qkv.clone()
    poisoned[sr.dead(T, lengths, N)] = float("nan")
    poisoned[..., ::2][sr.dead(T, lengths, N)] = float("inf")
    assert torch.equal(run_self(poisoned, *args), got)


@pytest.mark.parametrize("i", range(len(cr.CASES)))
def test_cross_attention_cases(i):
    Tq, Tk, d, H, Hkv, _, N, _, ql, kl = cr.CASES[i]
    _, q, kv, _, scale, He = cr.case_operands(cr.CASES[i])
    got, lse = run_cross(q, kv, H, Hkv, scale, ql, kl, return_lse=True)
    check(got, lse, fr.cross_forward(q, kv, H, He, scale, ql, kl))
    assert torch.equal(run_cross(q, kv, H, Hkv, scale, ql, kl), got)
    if ql is None and kl is None:
        return
    for n, (Lq, Lk) in enumerate(cr.live_lengths(Tq, Tk, ql, kl, N)):
        assert bool((got[n, Lq:] == 0).all()), n
        if Lq > 0:
            alone = run_cross(q[n:n + 1, :Lq].contiguous(), kv[n:n + 1, :Lk].contiguous(), H, Hkv, scale, None, None)
            assert torch.equal(got[n, :Lq], alone[0]), (n, Lq, Lk)
    dq, dk = cr.dead(Tq, Tk, ql, kl, N)
    q2, kv2 = q.clone(), kv.clone()
    q2[dq], kv2[dk] = float("nan"), float("nan")
    kv2[..., ::2][dk] = float("-inf")
    assert torch.equal(run_cross(q2, kv2, H, Hkv, scale, ql, kl), got)


@pytest.mark.parametrize("which", ["qkv", "table", "q", "kv"])
def test_operand_four_bytes_off_a_16_byte_boundary(which):
    if which in ("qkv", "table"):
        T, d, H, Hkv, lengths = 40, 64, 4, 2, (40, 31)
        table = sr.make_table("normal", 5, H, T)
        _, qkv, _, scale = sr.make_case(21, 1, 2, T, H, Hkv, d, None, True, lengths, 33, 2.0, table)
        ops = {"qkv": qkv.to(DEV), "table": table.to(DEV)}
        call = lambda: kernels.attention_forward(ops["qkv"], H, scale, True, num_kv_heads=Hkv, lengths=lengths, window=33,   # noqa: E731
                                                 softcap=2.0, bias=ops["table"], return_lse=True)
        ref = fr.self_forward(qkv, H, Hkv, scale, True, lengths, 33, 2.0, table)
    else:
        _, q, kv, _, scale = cr.make_case(22, 1, 2, 40, 70, 4, 2, 64, None, (40, 31), (70, 33))
        ops = {"q": q.to(DEV), "kv": kv.to(DEV)}
        call = lambda: kernels.cross_attention_forward(ops["q"], ops["kv"], 4, scale, num_kv_heads=2, query_lengths=(40, 31),   # noqa: E731
                                                       key_lengths=(70, 33), return_lse=True)
        ref = fr.cross_forward(q, kv, 4, 2, scale, (40, 31), (70, 33))
    aligned = call()
    ops[which] = sr.misaligned(ops[which])
    got = call()
    check(*got, ref)
    assert torch.equal(got[0], aligned[0]) and torch.equal(got[1], aligned[1])


def test_no_t_by_t_allocation_in_forward_and_backward():
    """N = 1, H = 4, d = 64, T = 2048: one [N, H, T, T] fp32 tensor is 64 MiB, input and output together 6 MiB."""
    H, d, T = 4, 64, 2048
    one = H * T * T * 4
    qkv = torch.randn(1, T, 3 * H * d, device=DEV)
    peaks = {}
    for fused in (True, False):
        x = qkv.clone().requires_grad_()
        module = ScaledDotProductAttention(H, causal=True, fused_forward=fused)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        module(x).sum().backward()
        torch.cuda.synchronize()
        peaks[fused] = torch.cuda.max_memory_allocated() - before
        assert x.grad is not None and bool(torch.isfinite(x.grad).all())
    print(f"peak above the operands: fused {peaks[True] / 2**20:.1f} MiB, torch formula {peaks[False] / 2**20:.1f} MiB")
    assert peaks[True] < one, peaks
    assert peaks[False] > one, peaks   # the control
