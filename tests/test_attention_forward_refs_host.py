"""The bound of tests/attention_forward_refs.py is one the reference itself keeps: on every case of the two lists the modules' own
torch formula in fp32 on the CPU lies within it of the fp64 result; and ``fused_forward=True`` changes no byte on CPU tensors."""
import pytest
import torch

import attention_cross_refs as cr
import attention_forward_refs as fr
import attention_scoremod_refs as sr
from vivit_amd.backend import ScaledDotProductAttention, ScaledDotProductCrossAttention


def self_module(case, table, scale, **kw):
    T, d, H, Hkv, V, N, causal, _, lengths, window, cap, _ = case
    module = ScaledDotProductAttention(H, causal=causal, scale=scale, num_kv_heads=Hkv, window=window, softcap=cap, bias=table, **kw)
    module.set_lengths(lengths)
    return module


def cross_module(case, scale, **kw):
    module = ScaledDotProductCrossAttention(case[3], scale=scale, num_kv_heads=case[4], **kw)
    module.set_lengths(case[8], case[9])
    return module


@pytest.mark.parametrize("i", range(len(sr.CASES)))
def test_self_attention_formula_within_the_bound(i):
    case = sr.CASES[i]
    _, qkv, _, scale, He, table = sr.case_operands(case)
    ref, bound, _, _ = fr.self_forward(qkv, case[2], He, scale, case[6], case[8], case[9], case[10], table)
    got = self_module(case, table, scale)(qkv)
    print(f"max error / bound = {((got.double() - ref).abs() / bound).max().item():.3g}")
    ok, msg = fr.within(got, ref, bound)
    assert ok, msg
    assert torch.equal(self_module(case, table, scale, fused_forward=True)(qkv), got)


@pytest.mark.parametrize("i", range(len(cr.CASES)))
def test_cross_attention_formula_within_the_bound(i):
    case = cr.CASES[i]
    _, q, kv, _, scale, He = cr.case_operands(case)
    ref, bound, _, _ = fr.cross_forward(q, kv, case[3], He, scale, case[8], case[9])
    got = cross_module(case, scale)(q, kv)
    print(f"max error / bound = {((got.double() - ref).abs() / bound).max().item():.3g}")
    ok, msg = fr.within(got, ref, bound)
    assert ok, msg
    assert torch.equal(cross_module(case, scale, fused_forward=True)(q, kv), got)
