"""``kernels.attention_bias_factor`` (csrc/attention.hip, ``vivit_attention_bias_factor_f32``: the diagonal owner and its fold) against
the fp64 reference under the derived bound of tests/attention_bias_refs.py, and the properties the entry promises: a padded sample
has the bytes of the sample cut to its length and run alone with the shifted index, and +0 where it is dead; NaN and inf at dead
positions reach nothing; the bytes of a (v, n) slice depend on nothing around it; misaligned operands, the table included; a constant
per head on the table moves the result within the bounds; one column for every distance sums to zero within the bound; an index value
outside ``[0, R)`` is skipped; no ``T x T`` allocation; argument errors before any launch.

On the commit before the feature every test of this file fails: there is no ``kernels.attention_bias_factor``."""
import pytest
import torch

import attention_bias_refs as br
import attention_scoremod_refs as sr
from vivit_amd import _lib, kernels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [f"{i}-T{c[0]}-d{c[1]}-H{c[2]}-{c[3]}-W{c[9]}-{'c' if c[6] else 'f'}-cap{c[10]}-{c[11]}{'-buckets' if c[12] else ''}"
       for i, c in enumerate(br.CASES)]


def run(M, qkv, out, H, Hkv, scale, causal, lengths, window, cap, table, index, R):
    return kernels.attention_bias_factor(M.to(DEV), qkv.to(DEV), out.to(DEV), H, scale, causal, table.to(DEV), index=index, width=R,
                                         num_kv_heads=Hkv, lengths=lengths, window=window, softcap=cap)


def check(Gb, M, qkv, out, H, Hkv, scale, causal, lengths, window, cap, table, index, R):
    """Within the bound of the reference and finite; returns (reference, bound)."""
    ref, bound = br.factor(M, qkv, out, H, Hkv, scale, causal, lengths, window, cap, table, index, R)
    got = Gb.cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    err = (got.double() - ref).abs()
    print(f"max error / bound = {(err / bound).max().item():.3g}, max error = {err.max().item():.3g}, max |reference| = {ref.abs().max().item():.3g}")
    ok, msg = br.within(got, ref, bound)
    assert ok, msg
    return ref, bound


def plus_zero(t):
    return bool((t.view(torch.int32) == 0).all())


@pytest.mark.parametrize("i", range(len(br.CASES)), ids=lambda i: IDS[i])
def test_cases(i):
    """Within the bound and finite; per sample the bytes of the truncated sample run alone with the shifted index, +0 for a dead
    sample; NaN / inf at the dead positions change no byte."""
    T, d, H, Hkv, V, N, causal, _, lengths, window, cap, _, _ = br.CASES[i]
    M, qkv, out, scale, He, _, table, index, R = br.case_operands(br.CASES[i])
    Gb = run(M, qkv, out, H, Hkv, scale, causal, lengths, window, cap, table, index, R)
    assert tuple(Gb.shape) == (V, N, H, R)
    check(Gb, M, qkv, out, H, He, scale, causal, lengths, window, cap, table, index, R)
    if lengths is None:
        return
    Gb = Gb.cpu()
    for n, L in enumerate(lengths):
        if L == 0:
            assert plus_zero(Gb[:, n]), n
            continue
        alone = run(M[:, n:n + 1, :L].contiguous(), qkv[n:n + 1, :L].contiguous(), out[n:n + 1, :L].contiguous(), H, Hkv, scale, causal, None,
                    window, cap, table[:, T - L:T + L - 1].contiguous(), index[T - L:T + L - 1], R)
        assert torch.equal(Gb[:, n].view(torch.int32), alone[:, 0].cpu().view(torch.int32)), (n, L)
    dead = br.dead(T, lengths, N)
    M2, q2, o2 = M.clone(), qkv.clone(), out.clone()
    M2[:, dead], o2[dead], q2[dead] = float("nan"), float("-inf"), float("nan")
    q2[..., ::2][dead] = float("inf")
    assert torch.equal(run(M2, q2, o2, H, Hkv, scale, causal, lengths, window, cap, table, index, R).cpu().view(torch.int32), Gb.view(torch.int32))


@pytest.mark.parametrize("d", [20, 64])
def test_bytes_do_not_depend_on_the_call_the_batch_or_the_chunk(d):
    V, N, T, H, Hkv, W, cap = 3, 4, 70, 4, 2, 33, 1.5
    lengths = (70, 33, 64, 1)
    table, index, R = sr.make_table("normal", d, H, T), torch.arange(2 * T - 1), 2 * T - 1
    args = (H, Hkv)
    M, qkv, out, scale = sr.make_case(11 + d, V, N, T, H, Hkv, d, None, True, lengths, W, cap, table)
    G1 = run(M, qkv, out, *args, scale, True, lengths, W, cap, table, index, R)
    assert torch.equal(G1, run(M, qkv, out, *args, scale, True, lengths, W, cap, table, index, R))
    other = run(M, qkv, out, *args, scale, True, (1, 70, 64, 0), W, cap, table, index, R)
    assert torch.equal(G1[:, 2], other[:, 2])
    alone = run(M[1:2, 2:3].contiguous(), qkv[2:3].contiguous(), out[2:3].contiguous(), *args, scale, True, lengths[2:3], W, cap, table, index, R)
    assert torch.equal(G1[1, 2], alone[0, 0])
    # rows of a later chunk, of a chunk's last place and of a ragged last chunk: chunks 4, 4, 1 (d = 20) and 2, 2, 1 (d = 64)
    V, rows = (9, (3, 4, 8)) if d == 20 else (5, (1, 2, 4))
    assert V == 2 * sr.chunk(d) + 1
    M, qkv, out, scale = sr.make_case(13 + d, V, N, T, H, Hkv, d, None, True, lengths, W, cap, table)
    G = run(M, qkv, out, *args, scale, True, lengths, W, cap, table, index, R)
    check(G, M, qkv, out, *args, scale, True, lengths, W, cap, table, index, R)
    for v in rows:
        alone = run(M[v:v + 1].contiguous(), qkv, out, *args, scale, True, lengths, W, cap, table, index, R)
        assert torch.equal(G[v], alone[0]), v


@pytest.mark.parametrize("which", ["M", "table"])
@pytest.mark.parametrize("d", [4, 20, 64, 128])
def test_operand_four_bytes_off_a_16_byte_boundary(d, which):
    V, N, T, H, Hkv, W, cap = 3, 2, 40, 3, 1, 33, 2.0
    lengths = (40, 31)
    table, index, R = sr.make_table("normal", d, H, T), torch.arange(2 * T - 1), 2 * T - 1
    M, qkv, out, scale = sr.make_case(17 + d, V, N, T, H, Hkv, d, None, True, lengths, W, cap, table)
    ops = {"M": M.to(DEV), "table": table.to(DEV)}
    qd, od = qkv.to(DEV), out.to(DEV)
    assert all(t.data_ptr() % 16 == 0 for t in ops.values())
    call = lambda: kernels.attention_bias_factor(ops["M"], qd, od, H, scale, True, ops["table"], index=index, width=R, num_kv_heads=Hkv,   # noqa: E731
                                                 lengths=lengths, window=W, softcap=cap)
    aligned = call()
    ops[which] = br.misaligned(ops[which])
    assert ops[which].data_ptr() % 16 == 4
    G = call()
    check(G, M, qkv, out, H, Hkv, scale, True, lengths, W, cap, table, index, R)
    assert torch.equal(G, aligned)


@pytest.mark.parametrize("cap", [None, 3.0])
@pytest.mark.parametrize("shift", [5.0, -5.0])
def test_a_constant_per_head_on_the_table_stays_within_the_two_bounds(shift, cap):
    V, N, T, H, Hkv, d = 3, 2, 70, 4, 2, 20
    lengths = (70, 40)
    table, index, R = sr.make_table("normal", 3, H, T), torch.arange(2 * T - 1), 2 * T - 1
    shifted = table + shift * torch.tensor([1.0, -1.0, 0.5, 1.0])[:, None]
    M, qkv, out, scale = sr.make_case(19, V, N, T, H, Hkv, d, None, False, lengths, None, cap, table)
    G0 = run(M, qkv, out, H, Hkv, scale, False, lengths, None, cap, table, index, R)
    G1 = run(M, qkv, out, H, Hkv, scale, False, lengths, None, cap, shifted, index, R)
    _, b0 = check(G0, M, qkv, out, H, Hkv, scale, False, lengths, None, cap, table, index, R)
    _, b1 = check(G1, M, qkv, out, H, Hkv, scale, False, lengths, None, cap, shifted, index, R)
    assert bool(((G0.cpu().double() - G1.cpu().double()).abs() <= b0 + b1).all())


@pytest.mark.parametrize("causal", [False, True])
def test_one_column_for_every_distance_is_zero_within_the_bound(causal):
    """The rows of dS sum to zero, so a bucket map that sends every distance to one column leaves a column of rounding errors."""
    V, N, T, H, Hkv, d = 3, 2, 70, 4, 2, 20
    lengths = (70, 33)
    table, index = sr.make_table("normal", 5, H, T), torch.zeros(2 * T - 1, dtype=torch.int64)
    M, qkv, out, scale = sr.make_case(29, V, N, T, H, Hkv, d, None, causal, lengths, None, 1.5, table)
    G = run(M, qkv, out, H, Hkv, scale, causal, lengths, None, 1.5, table, index, 1)
    ref, bound = check(G, M, qkv, out, H, Hkv, scale, causal, lengths, None, 1.5, table, index, 1)
    assert bool((ref.abs() <= bound).all()) and bool((G.cpu().double().abs() <= 2 * bound).all())
    wide, _ = br.factor(M, qkv, out, H, Hkv, scale, causal, lengths, None, 1.5, table, torch.arange(2 * T - 1), 2 * T - 1)
    assert wide.abs().max().item() > 1e3 * bound.max().item()                     # (the terms themselves are not small)


def test_an_index_value_outside_the_columns_is_skipped():
    """Visible distances with a column >= R or < 0 go nowhere; the other columns keep their bytes and the columns nothing else
    maps to are +0 (the contract: the fold skips such a value, nothing is stored for it)."""
    V, N, T, H, Hkv, d, R = 3, 2, 70, 4, 2, 20, 10
    lengths = (70, 33)
    table = sr.make_table("normal", 7, H, T)
    index = (torch.arange(2 * T - 1) // 3) % R                                     # every column is used by many distances
    M, qkv, out, scale = sr.make_case(31, V, N, T, H, Hkv, d, None, False, lengths, None, None, table)
    good = run(M, qkv, out, H, Hkv, scale, False, lengths, None, None, table, index, R)
    bad = index.clone()
    bad[index == 4] = R                      # the first value beyond
    bad[index == 7] = -1
    bad[T - 1] = (1 << 31) - 1               # the distance 0, which every sample sees; it belongs to column ((T - 1) // 3) % R
    got = run(M, qkv, out, H, Hkv, scale, False, lengths, None, None, table, bad, R)
    own = ((T - 1) // 3) % R
    keep = [b for b in range(R) if b not in (4, 7, own)]
    assert torch.equal(got[..., keep], good[..., keep])
    assert plus_zero(got[..., [4, 7]].cpu().contiguous())
    check(got, M, qkv, out, H, Hkv, scale, False, lengths, None, None, table, bad, R)


def test_no_t_by_t_allocation():
    V, N, T, H, Hkv, d, cap = 4, 2, 512, 4, 1, 16, 1.5
    lengths, W = torch.tensor([512, 100], dtype=torch.int32, device=DEV), 40
    table = sr.make_table("normal", 1, H, T)
    M, qkv, out, scale = sr.make_case(3, V, N, T, H, Hkv, d, None, False, (512, 100), W, cap, table)
    Md, qd, od, td = M.to(DEV), qkv.to(DEV), out.to(DEV), table.to(DEV)
    index = torch.arange(2 * T - 1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    G = kernels.attention_bias_factor(Md, qd, od, H, scale, False, td, index=index, width=2 * T - 1, num_kv_heads=Hkv, lengths=lengths,
                                      window=W, softcap=cap)
    torch.cuda.synchronize()
    assert tuple(G.shape) == (V, N, H, 2 * T - 1)
    extra = torch.cuda.max_memory_allocated() - before - G.numel() * 4
    scoremod = _lib.load().vivit_attention_scoremod_jac_t_f32_workspace_bytes(V, N, T, H, Hkv, d)
    print(f"peak beyond operands and result: {extra} bytes; the scoremod workspace: {scoremod}; 32 V N H T = {32 * V * N * H * T}")
    assert extra < 32 * V * N * H * T + scoremod, extra
    check(G, M, qkv, out, H, Hkv, scale, False, (512, 100), W, cap, table, index.cpu(), 2 * T - 1)


def test_argument_errors_come_before_any_launch():
    z = lambda *s: torch.zeros(*s, device=DEV)   # noqa: E731
    args = (z(1, 2, 3, 16), z(2, 3, 32), z(2, 3, 16), 4, 1.0, False)
    for cap in (0, -2.0, float("inf"), float("nan"), "1"):
        with pytest.raises(ValueError, match="softcap must be"):
            kernels.attention_bias_factor(*args, z(4, 5), num_kv_heads=2, softcap=cap)
    for bias in (z(4, 4), z(3, 5), z(4, 5, 1), z(20)):
        with pytest.raises(ValueError, match="bias must be"):
            kernels.attention_bias_factor(*args, bias, num_kv_heads=2)
    for bias in (torch.zeros(4, 5), z(4, 5).double()):
        with pytest.raises(RuntimeError):
            kernels.attention_bias_factor(*args, bias, num_kv_heads=2)
    for index in (torch.zeros(4, dtype=torch.int64), torch.zeros(5), torch.zeros(1, 5, dtype=torch.int32), torch.zeros(5, dtype=torch.bool)):
        with pytest.raises(ValueError, match="index must be"):
            kernels.attention_bias_factor(*args, z(4, 5), index=index, width=3, num_kv_heads=2)
    for width in (None, 0, -1, 2.5, True):
        with pytest.raises(ValueError, match="width must be"):
            kernels.attention_bias_factor(*args, z(4, 5), index=torch.zeros(5, dtype=torch.int64), width=width, num_kv_heads=2)
    with pytest.raises(ValueError, match="width must be"):
        kernels.attention_bias_factor(*args, z(4, 5), width=7, num_kv_heads=2)
    with pytest.raises(ValueError, match="window must be"):
        kernels.attention_bias_factor(*args, z(4, 5), num_kv_heads=2, window=0)
    with pytest.raises(ValueError, match="lengths must be"):
        kernels.attention_bias_factor(*args, z(4, 5), num_kv_heads=2, lengths=[1, 2, 3])
    with pytest.raises(ValueError, match="out must be"):
        kernels.attention_bias_factor(z(1, 2, 3, 16), z(2, 3, 32), z(2, 3, 32), 4, 1.0, False, z(4, 5), num_kv_heads=2)
    with pytest.raises(ValueError, match="M must be"):
        kernels.attention_bias_factor(z(1, 2, 4, 16), z(2, 3, 32), z(2, 3, 16), 4, 1.0, False, z(4, 5), num_kv_heads=2)
    assert tuple(kernels.attention_bias_factor(*args, z(4, 5), num_kv_heads=2).shape) == (1, 2, 4, 5)   # (index=None: the identity)
