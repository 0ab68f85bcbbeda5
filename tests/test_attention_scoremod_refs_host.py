"""Host checks of tests/attention_scoremod_refs.py, of the attention modules' forward pass with ``softcap`` / ``bias`` and of the torch
restatement of the rule (no GPU).  The reference is the transposed Jacobian (fp64 autograd) of a module-free restatement of the
function and of the module's forward pass; a constant added to a head's whole table changes nothing; a cap of 10^6 is the uncapped
reference within the bound; no modifier is the masked reference exactly; ``alibi_bias`` has the slopes of the paper; the rule the
factor provider uses for non-HIP tensors stays inside the derived bounds in fp32; the case list obeys its rule."""
import pytest
import torch

import attention_masked_refs as mr
import attention_scoremod_refs as sr
from vivit_amd import kernels
from vivit_amd.backend import MultiheadSelfAttention, ScaledDotProductAttention, SoftCap, alibi_bias
from vivit_amd.backend.extensions import _activation_kind, _attention_jac_t_torch

_REFS = {}
IDS = [f"{i}-T{c[0]}-d{c[1]}-H{c[2]}-{c[3]}-W{c[9]}-{'c' if c[6] else 'f'}-cap{c[10]}-{c[11]}" for i, c in enumerate(sr.CASES)]
SMALL = [i for i, c in enumerate(sr.CASES) if c[0] <= 33 or i % 7 == 0]


def operands(i):
    """The operands of case ``i`` as the GPU test makes them, with the fp64 reference (computed once, shared, never written to)."""
    if i not in _REFS:
        T, d, H, Hkv, V, N, causal, _, lengths, window, cap, _ = sr.CASES[i]
        M, qkv, out, scale, He, table = sr.case_operands(sr.CASES[i])
        _REFS[i] = (M, qkv, out, scale, He, table) + sr.rule(M, qkv, out, H, He, scale, causal, lengths, window, cap, table)
    return _REFS[i]


def module_for(case, scale, table, max_len=None):
    T, d, H, Hkv, V, N, causal, _, lengths, window, cap, _ = case
    if table is not None and max_len is not None:   # the case's table in the middle of a longer one
        longer = torch.randn(H, 2 * max_len - 1, generator=sr.gen(5)) * 3.0
        longer[:, max_len - T:max_len + T - 1] = table
        table = longer
    module = ScaledDotProductAttention(H, causal=causal, scale=scale, num_kv_heads=Hkv, window=window, softcap=cap, bias=table)
    module.set_lengths(None if lengths is None else list(lengths))
    return module


def plain_function(qkv, H, Hkv, scale, vis, cap, table):
    """The function restated without the module and without the reference's helpers: a loop over the heads, K and V of head h // R,
    the table gathered by j - i + T - 1.  ``vis [N, T, T]`` bool; rows without a visible key give zeros."""
    N, T, W = qkv.shape
    d, R = W // (H + 2 * Hkv), H // Hkv
    idx = torch.arange(T)[None, :] - torch.arange(T)[:, None] + T - 1            # [i, j] -> j - i + T - 1
    outs = []
    for h in range(H):
        g = h // R
        q, k = qkv[..., h * d:(h + 1) * d], qkv[..., (H + g) * d:(H + g + 1) * d]
        v = qkv[..., (H + Hkv + g) * d:(H + Hkv + g + 1) * d]
        s = scale * torch.einsum("nic,njc->nij", q, k)
        if cap is not None:
            s = cap * torch.tanh(s / cap)
        if table is not None:
            s = s + table[h].to(s.dtype)[idx]
        some = vis.any(-1, keepdim=True)                                          # (an empty row looks at itself, then is zeroed)
        p = s.masked_fill(~(vis | (~some & torch.eye(T, dtype=torch.bool))), float("-inf")).softmax(-1)
        outs.append((p * some) @ v)
    return torch.cat(outs, -1)


@pytest.mark.parametrize("i", SMALL, ids=lambda i: IDS[i])
def test_reference_is_the_transposed_jacobian_of_the_restated_function_and_of_the_module(i):
    case = sr.CASES[i]
    T, d, H, Hkv, V, N, causal, _, lengths, window, cap, _ = case
    M, qkv, out, scale, He, table, ref, bound = operands(i)
    dead = mr.dead(T, lengths, N)
    vis = mr.visible(T, lengths, causal, window).expand(N, T, T)
    x = qkv.double().masked_fill(dead[:, :, None], 0.0).requires_grad_(True)
    y = plain_function(x, H, He, scale, vis, cap, table)
    assert (y.detach() - sr.forward(qkv.double(), H, He, scale, causal, lengths, window, cap, table)).abs().max().item() <= 1e-12 * max(
        1.0, y.abs().max().item())
    ref64, _ = sr.rule(M, qkv, y.detach(), H, He, scale, causal, lengths, window, cap, table)
    module = module_for(case, scale, table)
    xm = qkv.double().requires_grad_(True)
    ym = module.double()(xm)
    assert (ym - y).abs().max().item() <= 1e-12 * max(1.0, y.abs().max().item())
    for vi in range(V):
        (g,) = torch.autograd.grad(y, x, M[vi].double().masked_fill(dead[:, :, None], 0.0), retain_graph=True)
        (gm,) = torch.autograd.grad(ym, xm, M[vi].double(), retain_graph=True)
        tol = 1e-11 * max(1.0, ref64[vi].abs().max().item())
        assert bool(torch.isfinite(g).all()) and bool((ref64[vi][dead] == 0).all()) and bool((gm[dead] == 0).all())
        assert (g.masked_fill(dead[:, :, None], 0.0) - ref64[vi]).abs().max().item() <= tol
        assert (gm - ref64[vi]).abs().max().item() <= tol
    assert ((ref - ref64).abs() / bound).max().item() <= 1.0
    assert bool((bound[:, dead] == sr.FLT_MIN).all()) and bool((ref[:, dead] == 0).all())


@pytest.mark.parametrize("i", [i for i in SMALL if sr.CASES[i][11] is not None][:6], ids=lambda i: IDS[i])
def test_a_constant_per_head_on_the_whole_table_changes_nothing(i):
    T, d, H, Hkv, V, N, causal, _, lengths, window, cap, _ = sr.CASES[i]
    M, qkv, out, scale, He, table, ref, bound = operands(i)
    shifted = table.double() + torch.linspace(-5.0, 5.0, H, dtype=sr.F64)[:, None]
    f0 = sr.forward(qkv.double(), H, He, scale, causal, lengths, window, cap, table.double())
    f1 = sr.forward(qkv.double(), H, He, scale, causal, lengths, window, cap, shifted)
    assert (f0 - f1).abs().max().item() <= 1e-12 * max(1.0, f0.abs().max().item())
    ref1, _ = sr.rule(M, qkv, out, H, He, scale, causal, lengths, window, cap, shifted)
    assert (ref - ref1).abs().max().item() <= 1e-11 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("i", [i for i in SMALL if sr.CASES[i][10] is not None][:6], ids=lambda i: IDS[i])
def test_a_cap_of_a_million_is_the_uncapped_reference_within_the_bound(i):
    T, d, H, Hkv, V, N, causal, _, lengths, window, cap, _ = sr.CASES[i]
    M, qkv, _, scale, He, table = operands(i)[:6]
    out = sr.forward(qkv, H, He, scale, causal, lengths, window, None, table)
    free, bound = sr.rule(M, qkv, out, H, He, scale, causal, lengths, window, None, table)
    capped, bound_c = sr.rule(M, qkv, out, H, He, scale, causal, lengths, window, 1e6, table)
    assert ((capped - free).abs() / bound).max().item() <= 1.0 and ((capped - free).abs() / bound_c).max().item() <= 1.0


@pytest.mark.parametrize("i", range(0, len(mr.CASES), 5))
def test_no_modifier_is_the_masked_reference_exactly(i):
    T, d, H, Hkv, V, N, causal, _, lengths, window = mr.CASES[i]
    M, qkv, out, scale, He = mr.case_operands(mr.CASES[i])
    want, want_bound = mr.rule(M, qkv, out, H, He, scale, causal, lengths, window)
    got, bound = sr.rule(M, qkv, out, H, He, scale, causal, lengths, window)
    assert torch.equal(got, want) and torch.equal(bound, want_bound)
    assert torch.equal(sr.forward(qkv, H, He, scale, causal, lengths, window), out)


def test_alibi_bias_has_the_slopes_of_the_paper():
    # H = 8: 2^-1 .. 2^-8.  H = 12: the eight of H = 8, then the first, third, fifth and seventh of H = 16 (2^-0.5, 2^-1.5, 2^-2.5, 2^-3.5)
    slopes8 = [0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625, 0.0078125, 0.00390625]
    slopes12 = slopes8 + [0.7071067811865476, 0.35355339059327373, 0.17677669529663687, 0.08838834764831843]
    for H, slopes in ((8, slopes8), (12, slopes12)):
        L = 6
        table = alibi_bias(H, L)
        assert tuple(table.shape) == (H, 2 * L - 1) and table.dtype == torch.float32
        for h in range(H):
            for delta in range(-(L - 1), L):
                assert table[h, delta + L - 1].item() == pytest.approx(-slopes[h] * abs(delta), rel=1e-6, abs=0.0), (H, h, delta)
        assert bool((table[:, L - 1] == 0).all())
    assert alibi_bias(1, 3).tolist() == [[-0.0078125, -0.00390625, 0.0, -0.00390625, -0.0078125]]       # H = 1: 2^-8
    # as the matrix of a causal layer: row i, column j <= i holds -m (i - j)
    B = sr.bias_matrix(alibi_bias(8, 5), 5)
    assert B[2, 4, 1].item() == -0.125 * 3 and B[0, 3, 3].item() == 0.0


@pytest.mark.parametrize("i", range(len(sr.CASES)), ids=lambda i: IDS[i])
def test_torch_rule_of_the_module_stays_within_the_bounds(i):
    """``_attention_jac_t_torch`` in fp32 with the modifiers, and the module's forward pass; the table as the middle of a longer one."""
    case = sr.CASES[i]
    T, d, H, Hkv, V, N, causal, _, lengths, window, cap, _ = case
    M, qkv, out, scale, He, table, ref, bound = operands(i)
    assert ref.shape == bound.shape == (V, N, T, (H + 2 * He) * d) and bool((bound > 0).all())
    module = module_for(case, scale, table, max_len=T + 3 if i % 2 else None)
    fwd = module(qkv)
    assert fwd.shape == out.shape and (fwd - out).abs().max().item() <= 1e-5 * max(1.0, out.abs().max().item())
    got = _attention_jac_t_torch(module, M, qkv, out, module.forward_lengths)
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    assert bool((got[:, mr.dead(T, lengths, N)] == 0).all())
    ratio = ((got.double() - ref).abs() / bound).max().item()
    print(f"max error / bound = {ratio:.3g}")
    assert ratio <= 0.5, ratio


def test_the_cap_is_felt_and_a_dropped_derivative_is_caught():
    """On the capped cases that bend unit logits, the mean of t^2 is not negligible, and the rule without (1 - t^2) leaves the bound."""
    for i in SMALL:
        T, d, H, Hkv, V, N, causal, _, lengths, window, cap, _ = sr.CASES[i]
        if cap is None or cap > 5 or T < 5:
            continue
        M, qkv, out, scale, He, table, ref, bound = operands(i)
        assert sr.mean_t2(qkv, H, He, scale, cap) > 0.05
        module = module_for(sr.CASES[i], scale, table)
        module(qkv)
        dropped = _attention_jac_t_torch(_Unbent(module), M, qkv, out, module.forward_lengths)   # the right P, dS in the place of dZ
        assert ((dropped.double() - ref).abs() / bound).max().item() > 10.0, i


class _Unbent:
    """A stand-in for the module in ``_attention_jac_t_torch`` that caps the scores and reports no cap: P is right, (1 - t^2) is
    dropped."""

    def __init__(self, module):
        self._m = module

    def __getattr__(self, name):
        return None if name == "softcap" else getattr(self._m, name)


def test_module_arguments():
    for bad in (0, -1.0, float("inf"), float("nan"), "2", True):
        with pytest.raises(ValueError, match="softcap"):
            ScaledDotProductAttention(2, softcap=bad)
        with pytest.raises(ValueError, match="softcap"):
            SoftCap(bad)
        with pytest.raises(ValueError, match="softcap"):
            kernels.attention_jac_t(torch.zeros(1, 1, 3, 4), torch.zeros(1, 3, 12), torch.zeros(1, 3, 4), 2, 1.0, False, softcap=bad)
        with pytest.raises(ValueError, match="softcap"):
            kernels.act_jac_t(torch.zeros(1, 3), torch.zeros(3), "softcap", bad)
    with pytest.raises(ValueError):
        SoftCap(None)
    for bad in (torch.zeros(3, 5), torch.zeros(2, 4), torch.zeros(2, 5, 1), torch.zeros(2, 5, dtype=torch.int64), [[0.0] * 5] * 2):
        with pytest.raises(ValueError, match="bias must be"):
            ScaledDotProductAttention(2, bias=bad)
    for poison in (float("nan"), float("inf"), float("-inf")):
        table = torch.zeros(2, 5)
        table[1, 3] = poison
        with pytest.raises(ValueError, match="finite"):
            ScaledDotProductAttention(2, bias=table)
    table = torch.randn(2, 9)
    module, given = ScaledDotProductAttention(2, bias=table, softcap=30), table.clone()
    table += 1.0                                                                    # the module keeps a copy
    assert "bias" in dict(module.named_buffers()) and not list(module.parameters()) and module.softcap == 30.0
    assert torch.equal(module.bias, given) and module.double().bias.dtype == torch.float64
    module = ScaledDotProductAttention(2, bias=table)
    assert tuple(module.bias_for(5).shape) == (2, 9) and torch.equal(module.bias_for(3), table[:, 2:7])
    assert torch.equal(module.bias_for(1), table[:, 4:5]) and ScaledDotProductAttention(2).bias_for(7) is None
    module(torch.randn(2, 5, 12))
    with pytest.raises(ValueError, match="at most 5"):
        module(torch.randn(2, 6, 12))
    block = MultiheadSelfAttention(8, 2, bias=alibi_bias(2, 7), causal=True, softcap=2.0)
    assert block[0].bias is not None and block[2].bias is not None and tuple(block[1].bias.shape) == (2, 13) and block[1].softcap == 2.0
    block = MultiheadSelfAttention(8, 2, bias=False, attention_bias=alibi_bias(2, 7))
    assert block[0].bias is None and tuple(block[1].bias.shape) == (2, 13)
    with pytest.raises(ValueError, match="two bias tables"):
        MultiheadSelfAttention(8, 2, bias=alibi_bias(2, 7), attention_bias=alibi_bias(2, 7))
    plain = MultiheadSelfAttention(8, 2)
    assert plain[1].bias is None and plain[1].softcap is None and plain[0].bias is not None
    cap = SoftCap(1.5)
    x = torch.linspace(-9, 9, 13)
    assert torch.equal(cap(x), 1.5 * torch.tanh(x / 1.5)) and _activation_kind(cap) == ("softcap", 1.5)
    assert kernels.ACTIVATION_KINDS["softcap"] == 10 and sorted(kernels.ACTIVATION_KINDS.values()) == list(range(11))


def test_the_rule_of_the_case_list_holds():
    C = sr.CASES
    assert len(set(C)) == len(C) and 24 <= len(C) <= 32
    for lo, hi in mr.INSTANCES:
        mine = [c for c in C if lo <= c[1] <= hi]
        VC = sr.chunk(lo)
        assert {lo, hi} <= {c[1] for c in mine} and {VC - 1, 2 * VC + 1} <= {c[4] for c in mine}
    assert any(c[3] is None for c in C) and {1, 2, 4} <= {c[2] // c[3] for c in C if c[3] is not None}
    assert {c[0] for c in C} == set(sr.T_ALL)
    kinds = {"cap": [c for c in C if c[10] is not None and c[11] is None], "table": [c for c in C if c[10] is None and c[11] is not None],
             "both": [c for c in C if c[10] is not None and c[11] is not None]}
    assert sum(len(v) for v in kinds.values()) == len(C)
    for name, mine in kinds.items():
        assert any(c[6] for c in mine) and any(not c[6] for c in mine), name
        assert {2, 33, 65} <= {c[9] for c in mine}, name
        assert any(c[8] is not None and 0 in c[8] and c[0] in c[8] and len(set(c[8])) > 2 for c in mine), name
    assert any(c[7] is not None and c[7] < 0 for c in C)
    assert any(c[11] == "alibi" for c in C) and any(c[11] == "normal" for c in C)
    assert all(c[0] <= 161 and c[2] <= 6 and c[1] <= 128 and c[4] <= 9 and c[5] <= 4 for c in C)
    assert any((c[0], c[1], c[2], c[5]) == (161, 128, 6, 4) for c in C)
    assert all(c[8] is None or len(c[8]) == c[5] for c in C)
