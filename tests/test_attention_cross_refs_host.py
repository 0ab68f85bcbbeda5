"""Host checks of tests/attention_cross_refs.py, of the cross-attention module's forward pass and of the torch restatement of the rule
(no GPU).  The reference is the transposed Jacobian (fp64 autograd) of an independently written forward pass -- a loop over the query
heads on ``repeat_interleave``d K and V -- on the live part and zero on the dead part; the fp32 torch rule the factor provider uses
for non-HIP tensors stays inside the derived bounds on every case; the module's forward pass is torch's own attention on the unpadded
cases, finite for any lengths and exactly zero at dead queries; the case list obeys its rule."""
import pytest
import torch
import torch.nn.functional as F

import attention_cross_refs as cr
from vivit_amd.backend import ScaledDotProductCrossAttention
from vivit_amd.backend.extensions import _cross_attention_jac_t_torch

IDS = [f"{i}-Tq{c[0]}-Tk{c[1]}-d{c[2]}-H{c[3]}-{c[4]}" for i, c in enumerate(cr.CASES)]


def module_for(case, scale):
    Tq, Tk, d, H, Hkv, V, N, _, ql, kl = case
    module = ScaledDotProductCrossAttention(H, scale=scale, num_kv_heads=Hkv)
    module.set_lengths(None if ql is None else list(ql), None if kl is None else list(kl))
    return module


def loop_forward(q, kv, H, Hkv, scale, lengths):
    """An independent forward pass: sample by sample on the live part, K and V copied to ``H`` heads, one softmax per query head.  Rows
    of dead queries stay zero (and take no part in the graph)."""
    N, Tq, E = q.shape
    d, R = E // H, H // Hkv
    rows = []
    for n, (Lq, Lk) in enumerate(lengths):
        out = torch.zeros(Tq, E, dtype=q.dtype)
        if Lq > 0:
            k = kv[n, :Lk, :Hkv * d].reshape(Lk, Hkv, d).repeat_interleave(R, 1)
            v = kv[n, :Lk, Hkv * d:].reshape(Lk, Hkv, d).repeat_interleave(R, 1)
            heads = []
            for h in range(H):
                s = (q[n, :Lq, h * d:(h + 1) * d] @ k[:, h].T) * scale
                heads.append(torch.softmax(s, -1) @ v[:, h])
            out = torch.cat((torch.cat(heads, 1), out[Lq:]), 0)
        rows.append(out)
    return torch.stack(rows)


def test_the_case_list_obeys_its_rule():
    assert max(max(c[0], c[1]) for c in cr.CASES) == 161 and max(c[3] for c in cr.CASES) == 6 and max(c[5] for c in cr.CASES) == 9
    assert max(c[6] for c in cr.CASES) == 4 and sum(c[7] is not None and c[7] < 0 for c in cr.CASES) == 1
    assert any(c[8] is None and c[9] is None for c in cr.CASES) and any(c[8] is None and c[9] is not None for c in cr.CASES)
    assert any(c[8] is not None and c[9] is None for c in cr.CASES)
    assert any(c[9] is not None and c[8] is not None and any(k == 0 and q > 0 for q, k in zip(c[8], c[9])) for c in cr.CASES)
    assert any(c[8] is not None and c[9] is not None and not any(c[8]) and not any(c[9]) for c in cr.CASES)
    drawn = {l for c in cr.CASES for l in (c[8] or ()) + (c[9] or ())}
    assert set(cr.LENGTHS) <= drawn and drawn <= set(cr.LENGTHS) | {5, 97, 161}


def test_dead_positions_are_the_definition():
    dq, dk = cr.dead(4, 6, (3, 4, 2, 9), (6, 0, -1, 2), 4)
    assert dq.tolist() == [[False, False, False, True], [True] * 4, [True] * 4, [False] * 4]
    assert dk.tolist() == [[False] * 6, [True] * 6, [True] * 6, [False, False, True, True, True, True]]
    assert cr.live_lengths(4, 6, None, (0, 3), 2) == [(0, 0), (4, 3)]


@pytest.mark.parametrize("i", range(len(cr.CASES)), ids=lambda i: IDS[i])
def test_module_forward(i):
    """Finite for any lengths, exact zeros at dead queries, the reference's forward pass, and the lengths kept as int32; on the
    unpadded cases torch's own attention (the tolerance of the forward comparison of tests/test_attention_layers.py)."""
    case = cr.CASES[i]
    Tq, Tk, d, H, Hkv, V, N, _, ql, kl = case
    M, q, kv, out, scale, He = cr.case_operands(case)
    module = module_for(case, scale)
    got = module(q.double(), kv.double())
    dq, _ = cr.dead(Tq, Tk, ql, kl, N)
    assert bool(torch.isfinite(got).all()) and bool((got[dq] == 0).all()) and bool((out[dq] == 0).all())
    assert (got - cr.forward(q.double(), kv.double(), H, He, scale, ql, kl)).abs().max().item() <= 1e-12 * max(1.0, got.abs().max().item())
    for kept, given in ((module.forward_query_lengths, ql), (module.forward_key_lengths, kl)):
        assert kept is None if given is None else (kept.dtype == torch.int32 and kept.tolist() == list(given))
    if ql is None and kl is None:
        R = H // He
        qh = q.double().view(N, Tq, H, d).transpose(1, 2)
        k = kv.double()[..., :He * d].reshape(N, Tk, He, d).transpose(1, 2).repeat_interleave(R, 1)
        v = kv.double()[..., He * d:].reshape(N, Tk, He, d).transpose(1, 2).repeat_interleave(R, 1)
        ref = F.scaled_dot_product_attention(qh, k, v, scale=scale).transpose(1, 2).reshape(N, Tq, H * d)
        assert ((got - ref).abs().max() / ref.abs().max()).item() <= 1e-12


@pytest.mark.parametrize("i", range(len(cr.CASES)), ids=lambda i: IDS[i])
def test_reference_is_the_transposed_jacobian_of_an_independent_forward(i):
    case = cr.CASES[i]
    Tq, Tk, d, H, Hkv, V, N, _, ql, kl = case
    M, q, kv, out, scale, He = cr.case_operands(case)
    Gq, bq, Gkv, bkv = cr.case_rule(case)
    x, z = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    y = loop_forward(x, z, H, He, scale, cr.live_lengths(Tq, Tk, ql, kl, N))
    assert (y.detach() - out.double()).abs().max().item() <= 1e-5 * max(1.0, out.abs().max().item())
    # the reference takes the fp32 module output as an input: hand it the fp64 one for this comparison
    Rq, _, Rkv, _ = cr.rule(M, q, kv, y.detach(), H, He, scale, ql, kl)
    dq, dk = cr.dead(Tq, Tk, ql, kl, N)
    for vi in range(V):
        if y.requires_grad:
            gq, gkv = torch.autograd.grad(y, (x, z), M[vi].double(), retain_graph=True, allow_unused=True)
            gq = torch.zeros_like(x) if gq is None else gq
            gkv = torch.zeros_like(z) if gkv is None else gkv
        else:   # (every query is dead: the output depends on nothing)
            gq, gkv = torch.zeros_like(x), torch.zeros_like(z)
        assert bool(torch.isfinite(gq).all()) and bool(torch.isfinite(gkv).all())
        assert bool((gq[dq] == 0).all()) and bool((gkv[dk] == 0).all())
        assert (gq - Rq[vi]).abs().max().item() <= 1e-11 * max(1.0, Rq[vi].abs().max().item())
        assert (gkv - Rkv[vi]).abs().max().item() <= 1e-11 * max(1.0, Rkv[vi].abs().max().item())
    assert ((Gq - Rq).abs() / bq).max().item() <= 1.0 and ((Gkv - Rkv).abs() / bkv).max().item() <= 1.0
    assert bool((bq[:, dq] == cr.FLT_MIN).all()) and bool((Gq[:, dq] == 0).all())
    assert bool((bkv[:, dk] == cr.FLT_MIN).all()) and bool((Gkv[:, dk] == 0).all())


@pytest.mark.parametrize("i", range(len(cr.CASES)), ids=lambda i: IDS[i])
def test_torch_rule_fp32_within_bounds(i):
    case = cr.CASES[i]
    Tq, Tk, d, H, Hkv, V, N, _, ql, kl = case
    M, q, kv, out, scale, He = cr.case_operands(case)
    Gq, bq, Gkv, bkv = cr.case_rule(case)
    module = module_for(case, scale)
    got = module(q, kv)                             # (sets the forward lengths; the module's fp32 forward is the reference's)
    assert (got - out).abs().max().item() <= 1e-5 * max(1.0, out.abs().max().item())
    lengths = (module.forward_query_lengths, module.forward_key_lengths)
    gq, gkv = _cross_attention_jac_t_torch(module, M, q, kv, out, *lengths)
    for got, ref, bound, dead in ((gq, Gq, bq, cr.dead(Tq, Tk, ql, kl, N)[0]), (gkv, Gkv, bkv, cr.dead(Tq, Tk, ql, kl, N)[1])):
        assert got.dtype == torch.float32 and got.shape == ref.shape and bool(torch.isfinite(got).all())
        ok, msg = cr.within(got, ref, bound)
        assert ok, msg
        assert bool((got[:, dead] == 0).all())
    only_q, only_kv = (_cross_attention_jac_t_torch(module, M, q, kv, out, *lengths, want=w) for w in ((True, False), (False, True)))
    assert only_q[1] is None and only_kv[0] is None and torch.equal(only_q[0], gq) and torch.equal(only_kv[1], gkv)


def test_reference_and_rule_ignore_the_data_of_dead_positions():
    case = cr.CASES[8]
    Tq, Tk, d, H, Hkv, V, N, _, ql, kl = case
    M, q, kv, out, scale, He = cr.case_operands(case)
    dq, dk = cr.dead(Tq, Tk, ql, kl, N)
    assert bool(dq.any()) and bool(dk.any())
    M2, q2, kv2, o2 = M.clone(), q.clone(), kv.clone(), out.clone()
    M2[:, dq], q2[dq], kv2[dk], o2[dq] = float("nan"), float("inf"), float("nan"), float("-inf")
    for a, b in zip(cr.rule(M2, q2, kv2, o2, H, He, scale, ql, kl), cr.case_rule(case)):
        assert torch.equal(a, b)
    module = module_for(case, scale)
    assert torch.equal(module(q2, kv2), module(q, kv))
    lengths = (module.forward_query_lengths, module.forward_key_lengths)
    for a, b in zip(_cross_attention_jac_t_torch(module, M2, q2, kv2, o2, *lengths), _cross_attention_jac_t_torch(module, M, q, kv, out, *lengths)):
        assert torch.equal(a, b)


def test_lengths_contract():
    module = ScaledDotProductCrossAttention(2)
    q, kv = torch.rand(2, 3, 4), torch.rand(2, 5, 8)
    for bad in ([1.0, 2.0], [[1, 2]], torch.ones(2, dtype=torch.bool)):
        with pytest.raises(ValueError, match="must be integers"):
            module.set_lengths(bad, None)
        with pytest.raises(ValueError, match="must be integers"):
            module.set_lengths(None, bad)
    module.set_lengths([3, 4], None)
    with pytest.raises(ValueError, match=r"query_lengths must lie in \[0, T = 3\]"):
        module(q, kv)
    module.set_lengths(None, [5, -1])
    with pytest.raises(ValueError, match=r"key_lengths must lie in \[0, T = 5\]"):
        module(q, kv)
    module.set_lengths([3], [5])
    with pytest.raises(ValueError, match="the batch has 2 samples"):
        module(q, kv)
    module.set_lengths([3, 0], [0, 5])
    assert bool((module(q, kv) == 0).all())
    module.set_lengths(None, None)
    assert module(q, kv).abs().min().item() > 0 and module.forward_query_lengths is None and module.forward_key_lengths is None
    with pytest.raises(ValueError, match="expected keys and values"):
        module(q, torch.rand(2, 5, 6))
    with pytest.raises(ValueError, match="expected queries"):
        module(torch.rand(2, 3, 5), kv)
