"""The fp64 reference of tests/attention_bias_refs.py (the factor of a learned relative-position bias table) checked on the host,
without a GPU: it equals autograd's gradient of ``<M[v, n], out[n]>`` with respect to the table through
``ScaledDotProductAttention(learn_bias=True)`` in fp64 on every case; the columns of a sample sum to zero within the summed bound (the
rows of ``dS`` do); columns that no visible distance maps to are exact zeros; ``relative_position_buckets`` gives T5's buckets at the
pinned distances; and the torch formula of the factor provider stays within the bound in fp32.

On the commit before the feature every test of this file fails: the module has no ``learn_bias``, the backend no
``relative_position_buckets`` and the factor provider no ``_attention_bias_factor_torch``."""
import pytest
import torch

import attention_bias_refs as br
from vivit_amd.backend import ScaledDotProductAttention, relative_position_buckets

F64 = torch.float64
IDS = [f"{i}-T{c[0]}-d{c[1]}-H{c[2]}-{c[3]}-W{c[9]}-{'c' if c[6] else 'f'}-cap{c[10]}-{c[11]}{'-buckets' if c[12] else ''}"
       for i, c in enumerate(br.CASES)]
_CACHE = {}


def reference(i):
    """Operands, reference and bound of case ``i``: computed once, shared by the tests below, never written to."""
    if i not in _CACHE:
        T, d, H, Hkv, V, N, causal, _, lengths, window, cap, _, _ = br.CASES[i]
        M, qkv, out, scale, He, param, table, index, R = br.case_operands(br.CASES[i])
        _CACHE[i] = (M, qkv, out, scale, He, param, table, index, R) + br.factor(M, qkv, out, H, He, scale, causal, lengths, window, cap,
                                                                                 table, index, R)
    return _CACHE[i]


def module_of(case, scale, param, index, dtype):
    T, d, H, Hkv, V, N, causal, _, lengths, window, cap, _, bucketed = case
    module = ScaledDotProductAttention(H, causal=causal, scale=scale, num_kv_heads=Hkv, window=window, softcap=cap, bias=param.to(dtype),
                                       learn_bias=True, bias_index=index if bucketed else None).to(dtype)
    module.set_lengths(None if lengths is None else list(lengths))
    return module


@pytest.mark.parametrize("i", range(len(br.CASES)), ids=lambda i: IDS[i])
def test_reference_is_autograd_through_the_module(i):
    case = br.CASES[i]
    T, d, H, Hkv, V, N, causal, _, lengths, window, cap, _, _ = case
    M, qkv, _, scale, He, param, table, index, R, _, _ = reference(i)
    module = module_of(case, scale, param, index, F64)
    assert isinstance(module.bias, torch.nn.Parameter) and tuple(module.bias.shape) == (H, R)
    out = module(qkv.to(F64))
    Gb, _ = br.factor(M, qkv, out.detach(), H, He, scale, causal, lengths, window, cap, table, index, R)   # (the fp64 forward output)
    auto = torch.zeros_like(Gb)
    for v in range(V):
        for n in range(N):
            auto[v, n] = torch.autograd.grad((M[v, n].to(F64) * out[n]).sum(), module.bias, retain_graph=True)[0]
    err, ref = (Gb - auto).abs().max().item(), auto.abs().max().item()
    print(f"max |reference - autograd| = {err:.3g}, max |autograd| = {ref:.3g}")
    # 1e-9 relative; the reference forms dP - D explicitly, which cancels in fp64 where autograd gives an exact 0 (one live
    # position: P = 1, dP = D up to rounding), so the rounding of that difference, d terms of size |M| |v|, is allowed besides
    floor = 4 * d * torch.finfo(F64).eps * M.abs().max().item() * qkv.abs().max().item()
    assert err <= 1e-9 * ref + floor
    if T > 1 and (lengths is None or max(lengths) > 1):   # (one position alone: dS = 1 * (dO v - dO o) = 0)
        assert ref > 0


@pytest.mark.parametrize("i", range(len(br.CASES)), ids=lambda i: IDS[i])
def test_columns_sum_to_zero_and_invisible_columns_are_zero(i):
    T, d, H, Hkv, V, N, causal, _, lengths, window, cap, _, bucketed = br.CASES[i]
    *_, index, R, Gb, bound = reference(i)
    assert bool((Gb.sum(-1).abs() <= bound.sum(-1)).all())
    seen = br.visible_distances(T, lengths, causal, window)                       # [N | 1, 2 T - 1]
    for n in range(N):
        vis = seen[n if lengths is not None else 0]
        hit = torch.zeros(R, dtype=torch.bool)
        hit[index[vis]] = True
        assert bool((Gb[:, n][..., ~hit] == 0).all()), n
        if causal and not bucketed:                                               # every j > i
            assert not bool(hit[T:].any()) and bool((Gb[:, n, :, T:] == 0).all())


def test_pinned_buckets():
    """T5's buckets for 32 buckets and a maximum distance of 128, away from the boundaries of the logarithmic range."""
    L = 1001
    b = relative_position_buckets(L, 32, 128, True)
    assert b.dtype == torch.int64 and tuple(b.shape) == (2 * L - 1,)
    at = lambda r: int(b[r + L - 1])   # noqa: E731
    for r, want in ((0, 0), (-1, 1), (-7, 7), (-12, 9), (-24, 11), (-48, 13), (-100, 15), (-1000, 15), (1, 17), (12, 25)):
        assert at(r) == want, (r, at(r), want)
    assert int(b.min()) == 0 and int(b.max()) == 31
    u = relative_position_buckets(L, 32, 128, False)
    assert bool((u[L:] == 0).all()) and int(u[L - 1]) == 0 and int(u[L - 2]) == 1 and int(u.max()) == 31
    assert bool((u[:L - 1][1:] <= u[:L - 1][:-1]).all())                         # farther back: never a smaller bucket
    short = relative_position_buckets(40, 32, 128, True)
    assert torch.equal(short, b[L - 40:L + 39])                                   # the bucket of a distance does not depend on max_len


@pytest.mark.parametrize("i", range(len(br.CASES)), ids=lambda i: IDS[i])
def test_torch_formula_in_fp32_within_the_bound(i):
    from vivit_amd.backend.extensions import _attention_bias_factor_torch

    case = br.CASES[i]
    lengths = case[8]
    M, qkv, out, scale, He, param, table, index, R, Gb, bound = reference(i)
    module = module_of(case, scale, param, index, torch.float32)
    got = _attention_bias_factor_torch(module, M, qkv, out, None if lengths is None else torch.tensor(lengths, dtype=torch.int32))
    assert tuple(got.shape) == tuple(Gb.shape) and got.dtype == torch.float32 and not got.requires_grad
    print(f"max error / bound = {((got.double() - Gb).abs() / bound).max().item():.3g}")
    ok, msg = br.within(got, Gb, bound)
    assert ok, msg
