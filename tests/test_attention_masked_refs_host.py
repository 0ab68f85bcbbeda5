"""Host checks of tests/attention_masked_refs.py, of the attention modules' forward pass with ``window`` / ``set_lengths`` and of the
torch restatements of the rule (no GPU).  The reference is the transposed Jacobian (fp64 autograd) of the module's forward pass on the
live part and zero on the dead part; the forward pass is torch's own attention under the explicit boolean mask on the live rows and
exact zeros on the dead ones, in the multi-head and in the grouped-query branch; the rules the factor provider uses for non-HIP tensors
stay inside the derived bounds in fp32; a window of ``T`` or more and lengths that are all ``T`` are the unmasked function, byte for
byte; the case list obeys its rule."""
import pytest
import torch
import torch.nn.functional as F

import attention_masked_refs as mr
from vivit_amd.backend import MultiheadSelfAttention, ScaledDotProductAttention
from vivit_amd.backend.extensions import _attention_jac_t_torch

_REFS = {}
IDS = [f"{i}-T{c[0]}-d{c[1]}-H{c[2]}-{c[3]}-W{c[9]}-{'c' if c[6] else 'f'}" for i, c in enumerate(mr.CASES)]


def operands(i):
    """The operands of case ``i`` as the GPU test makes them, with the fp64 reference (computed once, shared, never written to)."""
    if i not in _REFS:
        T, d, H, Hkv, V, N, causal, _, lengths, window = mr.CASES[i]
        M, qkv, out, scale, He = mr.case_operands(mr.CASES[i])
        _REFS[i] = (M, qkv, out, scale, He) + mr.rule(M, qkv, out, H, He, scale, causal, lengths, window)
    return _REFS[i]


def module_for(case, scale):
    T, d, H, Hkv, V, N, causal, _, lengths, window = case
    module = ScaledDotProductAttention(H, causal=causal, scale=scale, num_kv_heads=Hkv, window=window)
    module.set_lengths(None if lengths is None else list(lengths))
    return module


def sdpa_forward(qkv, H, Hkv, scale, vis):
    """An independent forward pass: K and V copied to H heads, torch's own attention with the boolean mask ``vis [N, T, T]``."""
    N, T, W = qkv.shape
    d, R = W // (H + 2 * Hkv), H // Hkv
    q = qkv[..., :H * d].view(N, T, H, d).transpose(1, 2)
    k = qkv[..., H * d:(H + Hkv) * d].view(N, T, Hkv, d).transpose(1, 2).repeat_interleave(R, 1)
    v = qkv[..., (H + Hkv) * d:].view(N, T, Hkv, d).transpose(1, 2).repeat_interleave(R, 1)
    return F.scaled_dot_product_attention(q, k, v, attn_mask=vis[:, None], scale=scale).transpose(1, 2).reshape(N, T, H * d)


def test_the_mask_is_the_definition():
    for T, lengths, causal, window in ((7, (7, 3, 0), True, 3), (7, (5, 7), False, 2), (6, None, True, None), (6, None, False, 1),
                                       (40, (33, 40, 1), False, 34)):
        vis = mr.visible(T, lengths, causal, window)
        for n in range(vis.shape[0]):
            L = T if lengths is None else lengths[n]
            for i in range(T):
                for j in range(T):
                    want = i < L and j < L and (not causal or j <= i) and (window is None or (i - j < window and j - i < window))
                    assert bool(vis[n, i, j]) == want, (n, i, j)
            assert bool(vis[n].diagonal()[:L].all())                      # a live query always sees itself


@pytest.mark.parametrize("i", [i for i, c in enumerate(mr.CASES) if c[0] <= 65 or i % 4 == 0], ids=lambda i: IDS[i])
def test_forward_is_torch_attention_under_the_mask_and_zero_on_dead_rows(i):
    case = mr.CASES[i]
    T, d, H, Hkv, V, N, causal, _, lengths, window = case
    M, qkv, out, scale, He = operands(i)[:5]
    module = module_for(case, scale)
    got = module(qkv.double())
    dead = mr.dead(T, lengths, N)
    assert bool((got[dead] == 0).all()) and bool((out[dead] == 0).all()) and bool(torch.isfinite(got).all())
    vis = mr.visible(T, lengths, causal, window).expand(N, T, T) | dead[:, :, None]   # (torch's attention must not meet an empty row)
    want = sdpa_forward(qkv.double(), H, He, scale, vis)
    live = ~dead
    assert (got[live] - want[live]).abs().max().item() <= 1e-12 * max(1.0, want[live].abs().max().item()) if bool(live.any()) else True
    assert (got - mr.forward(qkv.double(), H, He, scale, causal, lengths, window)).abs().max().item() <= 1e-12 * max(1.0, got.abs().max().item())
    # the lengths of this forward pass stay on the module, as int32
    if lengths is None:
        assert module.forward_lengths is None
    else:
        assert module.forward_lengths.dtype == torch.int32 and module.forward_lengths.tolist() == list(lengths)


@pytest.mark.parametrize("i", [i for i, c in enumerate(mr.CASES) if c[0] <= 33 or i % 7 == 0], ids=lambda i: IDS[i])
def test_reference_is_the_transposed_jacobian_of_the_module_forward(i):
    case = mr.CASES[i]
    T, d, H, Hkv, V, N, causal, _, lengths, window = case
    M, qkv, out, scale, He, ref, bound = operands(i)
    module = module_for(case, scale)
    x = qkv.double().requires_grad_(True)
    y = module(x)
    # the reference takes the fp32 module output as an input: hand it the fp64 one for this comparison
    ref64, _ = mr.rule(M, qkv, y.detach(), H, He, scale, causal, lengths, window)
    dead = mr.dead(T, lengths, N)
    for vi in range(V):
        (g,) = torch.autograd.grad(y, x, M[vi].double(), retain_graph=True)
        assert bool(torch.isfinite(g).all()) and bool((g[dead] == 0).all()) and bool((ref64[vi][dead] == 0).all())
        assert (g - ref64[vi]).abs().max().item() <= 1e-11 * max(1.0, ref64[vi].abs().max().item())
    assert ((ref - ref64).abs() / bound).max().item() <= 1.0
    assert bool((bound[:, dead] == mr.FLT_MIN).all()) and bool((ref[:, dead] == 0).all())


def test_reference_ignores_the_data_of_dead_positions():
    T, d, H, Hkv, V, N, causal, _, lengths, window = case = mr.CASES[0]
    M, qkv, out, scale, He, ref, bound = operands(0)
    dead = mr.dead(T, lengths, N)
    assert bool(dead.any())
    M2, q2, o2 = M.clone(), qkv.clone(), out.clone()
    M2[:, dead], q2[dead], o2[dead] = float("nan"), float("inf"), float("nan")
    ref2, bound2 = mr.rule(M2, q2, o2, H, He, scale, causal, lengths, window)
    assert torch.equal(ref, ref2) and torch.equal(bound, bound2)
    module = module_for(case, scale)
    assert torch.equal(module(q2), module(qkv)) and torch.equal(module(qkv), out)
    got = _attention_jac_t_torch(module, M2, q2, o2, module.forward_lengths)
    assert torch.equal(got, _attention_jac_t_torch(module, M, qkv, out, module.forward_lengths))


@pytest.mark.parametrize("i", range(len(mr.CASES)), ids=lambda i: IDS[i])
def test_torch_rule_of_the_module_stays_within_the_bounds(i):
    """``_attention_jac_t_torch`` in fp32, multi-head and grouped-query branch, with the lengths the module's forward pass kept."""
    case = mr.CASES[i]
    T, d, H, Hkv, V, N, causal, _, lengths, window = case
    M, qkv, out, scale, He, ref, bound = operands(i)
    assert ref.shape == bound.shape == (V, N, T, (H + 2 * He) * d) and bool((bound > 0).all())
    module = module_for(case, scale)
    fwd = module(qkv)
    assert fwd.shape == out.shape and (fwd - out).abs().max().item() <= 1e-5 * max(1.0, out.abs().max().item())
    got = _attention_jac_t_torch(module, M, qkv, out, module.forward_lengths)
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    dead = mr.dead(T, lengths, N)
    assert bool((got[:, dead] == 0).all())
    ratio = ((got.double() - ref).abs() / bound).max().item()
    print(f"max error / bound = {ratio:.3g}")
    assert ratio <= 0.5, ratio


@pytest.mark.parametrize("Hkv", [None, 2])
@pytest.mark.parametrize("causal", [False, True])
def test_a_window_of_T_and_full_lengths_are_the_unmasked_rule_exactly(causal, Hkv):
    V, N, T, H, d = 3, 3, 40, 4, 20
    M, qkv, out, scale = mr.gr.make_case(11, V, N, T, H, H if Hkv is None else Hkv, d, None, causal)
    plain = ScaledDotProductAttention(H, causal=causal, num_kv_heads=Hkv)
    base_out, base = plain(qkv), _attention_jac_t_torch(plain, M, qkv, out)
    assert plain.forward_lengths is None
    for window, lengths in ((T, None), (T + 5, None), (None, [T] * N), (T, torch.full((N,), T))):
        module = ScaledDotProductAttention(H, causal=causal, num_kv_heads=Hkv, window=window)
        module.set_lengths(lengths)
        assert torch.equal(module(qkv), base_out)
        assert torch.equal(_attention_jac_t_torch(module, M, qkv, out, module.forward_lengths), base)
    module.set_lengths(None)                                              # and back
    assert torch.equal(module(qkv), base_out) and module.forward_lengths is None


def test_module_arguments():
    with pytest.raises(ValueError, match="window"):
        ScaledDotProductAttention(2, window=0)
    with pytest.raises(ValueError, match="window"):
        MultiheadSelfAttention(8, 2, window=-1)
    with pytest.raises(ValueError, match="window"):
        ScaledDotProductAttention(2, window=1.5)
    module = ScaledDotProductAttention(2)
    with pytest.raises(ValueError, match="integers"):
        module.set_lengths([1.0, 2.0])
    with pytest.raises(ValueError, match="integers"):
        module.set_lengths(torch.ones(2, 2, dtype=torch.int64))
    x = torch.randn(2, 5, 12)
    module.set_lengths([5, 3, 1])
    with pytest.raises(ValueError, match="3 lengths, the batch has 2"):
        module(x)
    for bad in ([6, 1], [-1, 2]):
        module.set_lengths(bad)
        with pytest.raises(ValueError, match=r"\[0, T = 5\]"):
            module(x)
    block = MultiheadSelfAttention(8, 2, causal=True, num_kv_heads=1, window=3)
    assert block[1].window == 3 and block[1].causal and block[1].num_kv_heads == 1
    block.set_lengths([4, 2])
    assert block[1]._lengths.tolist() == [4, 2]
    y = block(torch.randn(2, 5, 8))
    assert block[1].forward_lengths.tolist() == [4, 2] and bool(torch.isfinite(y).all())
    mha = torch.nn.MultiheadAttention(8, 2, batch_first=True)
    assert MultiheadSelfAttention.from_torch(mha, causal=True, window=2)[1].window == 2
    assert MultiheadSelfAttention.from_torch(mha)[1].window is None


def test_the_rule_of_the_case_list_holds():
    C = mr.CASES
    assert len(set(C)) == len(C) and 24 <= len(C) <= 48
    for lo, hi in mr.INSTANCES:
        mine = [c for c in C if lo <= c[1] <= hi]
        VC = mr.chunk(lo)
        assert lo % 4 != 0 and {lo, hi} <= {c[1] for c in mine}
        assert {VC - 1, 2 * VC + 1} <= {c[4] for c in mine}
    assert any(c[3] is None for c in C) and {1, 2, 4} <= {c[2] // c[3] for c in C if c[3] is not None}
    assert {c[0] for c in C} == set(mr.T_ALL)
    drawn = set()
    for T, lengths in ((c[0], c[8]) for c in C if c[8] is not None):
        assert all(l == T or (l in mr.LENGTHS and l < T) for l in lengths)
        drawn |= {"T" if l == T else l for l in lengths}
    assert drawn == set(mr.LENGTHS) | {"T"}
    assert any(c[8] is not None and len(set(c[8])) > 2 for c in C)                          # mixed within a batch
    assert any(c[8] is None for c in C) and any(c[8] is not None and set(c[8]) == {c[0]} for c in C)
    assert sum(1 for c in C if c[8] is not None and set(c[8]) == {0}) == 1
    for causal in (False, True):
        mine = [c for c in C if c[6] == causal]
        assert {1, 2, 31, 32, 33, 34, 64, 65} <= {c[9] for c in mine}
        assert any(c[9] == c[0] for c in mine) and any(c[9] == c[0] + 5 for c in mine) and any(c[9] is None for c in mine)
        for T in (97, 161):
            assert {32, 33, 34, 64, 65} <= {c[9] for c in mine if c[0] == T}
    assert any(c[7] is not None and c[7] < 0 for c in C)
    assert all(c[0] <= 161 and c[2] <= 6 and c[1] <= 128 and c[4] <= 9 and c[5] <= 4 for c in C)
    assert all(c[8] is None or len(c[8]) == c[5] for c in C)
