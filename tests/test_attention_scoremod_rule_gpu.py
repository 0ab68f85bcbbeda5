"""``kernels.attention_jac_t(..., softcap=, bias=)`` (csrc/attention.hip, ``vivit_attention_scoremod_jac_t_f32``) against the fp64
reference under the derived bounds of tests/attention_scoremod_refs.py, and the properties the rule promises: without a modifier the
bytes of the masked entry; a padded sample has the bytes of the sample cut to its length and run alone with the table's middle
slice; the bytes of a (v, n) slice depend on nothing around it; a constant per head on the table moves the result within the bounds;
saturated caps give finite results with the small dQ and dK the reference says; NaN and inf at dead positions reach nothing;
misaligned operands, the table included; no ``T x T`` allocation; and ``kernels.act_jac_t(kind="softcap")``."""
import pytest
import torch

import attention_scoremod_refs as sr
from vivit_amd import _lib, kernels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [f"{i}-T{c[0]}-d{c[1]}-H{c[2]}-{c[3]}-W{c[9]}-{'c' if c[6] else 'f'}-cap{c[10]}-{c[11]}" for i, c in enumerate(sr.CASES)]


def run(M, qkv, out, H, Hkv, scale, causal, lengths=None, window=None, cap=None, table=None):
    return kernels.attention_jac_t(M.to(DEV), qkv.to(DEV), out.to(DEV), H, scale, causal, num_kv_heads=Hkv, lengths=lengths, window=window,
                                   softcap=cap, bias=None if table is None else table.to(DEV))


def report(got, ref, bound, H, Hkv, d):
    for name, sl in (("dQ", slice(0, H * d)), ("dK", slice(H * d, (H + Hkv) * d)), ("dV", slice((H + Hkv) * d, (H + 2 * Hkv) * d))):
        err = (got[..., sl].double() - ref[..., sl]).abs()
        print(f"{name}: max error / bound = {(err / bound[..., sl]).max().item():.3g}, max error = {err.max().item():.3g}, "
              f"max |reference| = {ref[..., sl].abs().max().item():.3g}")


def check(G, M, qkv, out, H, Hkv, scale, causal, lengths, window, cap, table, ref_cap="same"):
    """Within the bounds of the reference (``ref_cap``: the cap of the reference where it is not the kernel's), finite, zero rows."""
    ref, bound = sr.rule(M, qkv, out, H, Hkv, scale, causal, lengths, window, cap if ref_cap == "same" else ref_cap, table)
    got = G.cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    report(got, ref, bound, H, Hkv, M.shape[-1] // H)
    ok, msg = sr.within(got, ref, bound)
    assert ok, msg
    assert bool((got[:, sr.dead(M.shape[2], lengths, M.shape[1])] == 0).all())
    return ref, bound


def poisoned(M, qkv, out, lengths):
    """Copies with NaN and +-inf at the dead positions (plain data)."""
    dead = sr.dead(M.shape[2], lengths, M.shape[1])
    M2, q2, o2 = M.clone(), qkv.clone(), out.clone()
    M2[:, dead], o2[dead] = float("nan"), float("-inf")
    q2[dead] = float("nan")
    q2[..., ::2][dead] = float("inf")
    return M2, q2, o2


@pytest.mark.parametrize("i", range(len(sr.CASES)), ids=lambda i: IDS[i])
def test_cases(i):
    """Within the bounds and finite; per sample the bytes of the truncated sample run alone with the middle slice of the table and
    exact zeros beyond; NaN / inf at the dead positions change no byte."""
    T, d, H, Hkv, V, N, causal, _, lengths, window, cap, _ = sr.CASES[i]
    M, qkv, out, scale, He, table = sr.case_operands(sr.CASES[i])
    G = run(M, qkv, out, H, Hkv, scale, causal, lengths, window, cap, table)
    check(G, M, qkv, out, H, He, scale, causal, lengths, window, cap, table)
    if lengths is None:
        return
    G = G.cpu()
    for n, L in enumerate(lengths):
        assert bool((G[:, n, L:] == 0).all()), n
        if L > 0:
            middle = None if table is None else table[:, T - L:T + L - 1].contiguous()
            alone = run(M[:, n:n + 1, :L].contiguous(), qkv[n:n + 1, :L].contiguous(), out[n:n + 1, :L].contiguous(), H, Hkv, scale, causal,
                        None, window, cap, middle)
            assert tuple(alone.shape) == (V, 1, L, G.shape[-1])
            assert torch.equal(G[:, n, :L], alone[:, 0].cpu()), (n, L)
    M2, q2, o2 = poisoned(M, qkv, out, lengths)
    assert torch.equal(run(M2, q2, o2, H, Hkv, scale, causal, lengths, window, cap, table).cpu(), G)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d,Hkv", [(20, None), (64, 2)])
def test_no_modifier_is_the_masked_entry_byte_for_byte(d, Hkv, causal):
    V, N, T, H, W = 3, 3, 70, 4, 34
    lengths = (70, 33, 0)
    He = H if Hkv is None else Hkv
    M, qkv, out, scale = sr.mr.make_case(11 + d, V, N, T, H, He, d, None, causal, lengths, W)
    Md, qd, od = M.to(DEV), qkv.to(DEV), out.to(DEV)
    ld = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    lib = _lib.load()
    ws_bytes = lib.vivit_attention_masked_jac_t_f32_workspace_bytes(V, N, T, H, He, d)
    assert ws_bytes == lib.vivit_attention_scoremod_jac_t_f32_workspace_bytes(V, N, T, H, He, d) > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    want, got = torch.full((V, N, T, (H + 2 * He) * d), 7.0, device=DEV), torch.full((V, N, T, (H + 2 * He) * d), 9.0, device=DEV)
    st = lib.vivit_attention_masked_jac_t_f32(Md.data_ptr(), qd.data_ptr(), od.data_ptr(), want.data_ptr(), V, N, T, H, He, d, scale,
                                              int(causal), ld.data_ptr(), W, ws.data_ptr(), ws_bytes, stream)
    assert st == 0
    st = lib.vivit_attention_scoremod_jac_t_f32(Md.data_ptr(), qd.data_ptr(), od.data_ptr(), got.data_ptr(), V, N, T, H, He, d, scale,
                                                int(causal), ld.data_ptr(), W, 0.0, None, ws.data_ptr(), ws_bytes, stream)
    assert st == 0
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(run(M, qkv, out, H, Hkv, scale, causal, lengths, W, None, None), want)      # the wrapper with both None


@pytest.mark.parametrize("d", [20, 64])
def test_bytes_do_not_depend_on_the_call_the_batch_or_the_chunk(d):
    V, N, T, H, Hkv, W, cap = 3, 4, 70, 4, 2, 33, 1.5
    lengths = (70, 33, 64, 1)
    table = sr.make_table("normal", d, H, T)
    M, qkv, out, scale = sr.make_case(11 + d, V, N, T, H, Hkv, d, None, True, lengths, W, cap, table)
    G1 = run(M, qkv, out, H, Hkv, scale, True, lengths, W, cap, table)
    assert torch.equal(G1, run(M, qkv, out, H, Hkv, scale, True, lengths, W, cap, table))
    # sample 2 with other lengths around it, and alone
    other = run(M, qkv, out, H, Hkv, scale, True, (1, 70, 64, 0), W, cap, table)
    assert torch.equal(G1[:, 2], other[:, 2])
    alone = run(M[1:2, 2:3].contiguous(), qkv[2:3].contiguous(), out[2:3].contiguous(), H, Hkv, scale, True, lengths[2:3], W, cap, table)
    assert torch.equal(G1[1, 2], alone[0, 0])
    # rows of a later chunk, of a chunk's last place and of a ragged last chunk: chunks 4, 4, 1 (d = 20) and 2, 2, 1 (d = 64)
    V, rows = (9, (3, 4, 8)) if d == 20 else (5, (1, 2, 4))
    assert V == 2 * sr.chunk(d) + 1
    M, qkv, out, scale = sr.make_case(13 + d, V, N, T, H, Hkv, d, None, True, lengths, W, cap, table)
    G = run(M, qkv, out, H, Hkv, scale, True, lengths, W, cap, table)
    check(G, M, qkv, out, H, Hkv, scale, True, lengths, W, cap, table)
    for v in rows:
        alone = run(M[v:v + 1].contiguous(), qkv, out, H, Hkv, scale, True, lengths, W, cap, table)
        assert torch.equal(G[v], alone[0]), v


@pytest.mark.parametrize("cap", [None, 3.0])
@pytest.mark.parametrize("shift", [5.0, -5.0])
def test_a_constant_per_head_on_the_table_stays_within_the_two_bounds(shift, cap):
    V, N, T, H, Hkv, d = 3, 2, 70, 4, 2, 20
    lengths = (70, 40)
    table = sr.make_table("normal", 3, H, T)
    shifted = table + shift * torch.tensor([1.0, -1.0, 0.5, 1.0])[:, None]
    M, qkv, out, scale = sr.make_case(19, V, N, T, H, Hkv, d, None, False, lengths, None, cap, table)
    G0, G1 = run(M, qkv, out, H, Hkv, scale, False, lengths, None, cap, table), run(M, qkv, out, H, Hkv, scale, False, lengths, None, cap, shifted)
    _, b0 = check(G0, M, qkv, out, H, Hkv, scale, False, lengths, None, cap, table)
    _, b1 = check(G1, M, qkv, out, H, Hkv, scale, False, lengths, None, cap, shifted)
    assert bool(((G0.cpu().double() - G1.cpu().double()).abs() <= b0 + b1).all())


@pytest.mark.parametrize("table_kind", [None, "normal"])
def test_saturated_cap(table_kind):
    """c = 0.5 and logits of some +-40: most |z / c| > 10, tanhf gives +-1 and the factor 1 - t^2 is exactly 0.  Finite, within the
    bounds, and dQ and dK as small as the reference says."""
    V, N, T, H, Hkv, d, cap = 3, 2, 40, 4, 2, 20, 0.5
    lengths, W = (40, 33), 9
    table = sr.make_table(table_kind, 5, H, T)
    M, qkv, out, scale = sr.make_case(7, V, N, T, H, Hkv, d, None, True, lengths, W, cap, table, qk_gain=6.0)
    Z = sr.gr.logits(qkv, H, Hkv, scale)
    saturated = ((Z / cap).abs() > 10).double().mean().item()
    assert saturated > 0.5
    G = run(M, qkv, out, H, Hkv, scale, True, lengths, W, cap, table)
    ref, _ = check(G, M, qkv, out, H, Hkv, scale, True, lengths, W, cap, table)
    # small: only the unsaturated pairs pass anything on to q and k, so against the rule of the uncapped function on the same data
    # the mean magnitude of dQ | dK shrinks at least by their share (the reference says by ten times more); the kernel follows it
    free, _ = sr.rule(M, qkv, out, H, Hkv, scale, True, lengths, W, None, table)
    qk, got = slice(0, (H + Hkv) * d), G.cpu().double()
    print(f"saturated {saturated:.3f}; mean |dQ, dK|: kernel {got[..., qk].abs().mean().item():.3g}, reference "
          f"{ref[..., qk].abs().mean().item():.3g}, uncapped {free[..., qk].abs().mean().item():.3g}")
    assert ref[..., qk].abs().mean().item() < (1.0 - saturated) * free[..., qk].abs().mean().item()
    assert got[..., qk].abs().mean().item() < 1.5 * ref[..., qk].abs().mean().item()
    assert got[..., (H + Hkv) * d:].abs().max().item() > 0                       # dV does not feel the cap's derivative


def test_a_wide_cap_is_the_uncapped_reference():
    """c = 10^4 on unit data: within the bounds of the reference WITHOUT a cap."""
    V, N, T, H, Hkv, d = 3, 2, 70, 4, 1, 33
    lengths = (70, 31)
    M, qkv, out, scale = sr.make_case(23, V, N, T, H, Hkv, d, None, True, lengths, None, None, None)
    check(run(M, qkv, out, H, Hkv, scale, True, lengths, None, 1e4, None), M, qkv, out, H, Hkv, scale, True, lengths, None, 1e4, None,
          ref_cap=None)


@pytest.mark.parametrize("which", ["M", "qkv", "table"])
@pytest.mark.parametrize("d", [4, 20, 64, 128])
def test_operand_four_bytes_off_a_16_byte_boundary(d, which):
    V, N, T, H, Hkv, W, cap = 3, 2, 40, 3, 1, 33, 2.0
    lengths = (40, 31)
    table = sr.make_table("normal", d, H, T)
    M, qkv, out, scale = sr.make_case(17 + d, V, N, T, H, Hkv, d, None, True, lengths, W, cap, table)
    ops = {"M": M.to(DEV), "qkv": qkv.to(DEV), "table": table.to(DEV)}
    od = out.to(DEV)
    assert all(t.data_ptr() % 16 == 0 for t in ops.values())
    call = lambda: kernels.attention_jac_t(ops["M"], ops["qkv"], od, H, scale, True, num_kv_heads=Hkv, lengths=lengths, window=W,   # noqa: E731
                                           softcap=cap, bias=ops["table"])
    aligned = call()
    ops[which] = sr.misaligned(ops[which])
    assert ops[which].data_ptr() % 16 == 4
    G = call()
    check(G, M, qkv, out, H, Hkv, scale, True, lengths, W, cap, table)
    assert torch.equal(G, aligned)


def test_no_t_by_t_allocation():
    V, N, T, H, Hkv, d, cap = 4, 2, 256, 4, 1, 16, 1.5
    lengths, W = torch.tensor([256, 100], dtype=torch.int32, device=DEV), 40
    table = sr.make_table("normal", 1, H, T)
    M, qkv, out, scale = sr.make_case(3, V, N, T, H, Hkv, d, None, False, (256, 100), W, cap, table)
    Md, qd, od, td = M.to(DEV), qkv.to(DEV), out.to(DEV), table.to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    G = kernels.attention_jac_t(Md, qd, od, H, scale, False, num_kv_heads=Hkv, lengths=lengths, window=W, softcap=cap, bias=td)
    torch.cuda.synchronize()
    assert tuple(G.shape) == (V, N, T, (H + 2 * Hkv) * d)
    extra = torch.cuda.max_memory_allocated() - before - G.numel() * 4
    assert extra < N * T * T, extra                                        # not even one byte per (n, i, j)
    check(G, M, qkv, out, H, Hkv, scale, False, (256, 100), W, cap, table)


def test_argument_errors_come_before_any_launch():
    z = lambda *s: torch.zeros(*s, device=DEV)   # noqa: E731
    args = (z(1, 2, 3, 16), z(2, 3, 32), z(2, 3, 16), 4, 1.0, False)
    for cap in (0, -2.0, float("inf"), float("nan"), "1"):
        with pytest.raises(ValueError, match="softcap must be"):
            kernels.attention_jac_t(*args, num_kv_heads=2, softcap=cap)
    for bias in (z(4, 4), z(3, 5), z(4, 5, 1), z(20)):
        with pytest.raises(ValueError, match="bias must be"):
            kernels.attention_jac_t(*args, num_kv_heads=2, bias=bias)
    for bias in (torch.zeros(4, 5), z(4, 5).double()):
        with pytest.raises(RuntimeError):
            kernels.attention_jac_t(*args, num_kv_heads=2, bias=bias)
    with pytest.raises(ValueError, match="out must be"):                  # the older checks still come
        kernels.attention_jac_t(z(1, 2, 3, 16), z(2, 3, 32), z(2, 3, 32), 4, 1.0, False, num_kv_heads=2, softcap=2.0, bias=z(4, 5))
    with pytest.raises(ValueError, match="softcap must be"):
        kernels.act_jac_t(z(1, 3), z(3), "softcap", 0.0)


@pytest.mark.parametrize("cap", [0.5, 30.0])
@pytest.mark.parametrize("numel", [1, 63, 64, 65, 4097])
def test_act_jac_t_softcap(numel, cap):
    """Inputs from 0 to past saturation (|x / cap| up to 20, where tanhf is +-1 and the derivative exactly 0)."""
    g = sr.gen(numel)
    V = 3
    x = (torch.rand(numel, generator=g) * 2 - 1) * 20.0 * cap
    x[::5] *= 0.01
    M = torch.randn(V, numel, generator=g) * 10.0 ** (torch.rand(V, numel, generator=g) * 2 - 1)
    got = kernels.act_jac_t(M.to(DEV), x.to(DEV), "softcap", cap).cpu()
    ref, bound = sr.act_softcap(M, x, cap)
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    print(f"max error / bound = {((got.double() - ref).abs() / bound).max().item():.3g}")
    ok, msg = sr.within(got, ref, bound)
    assert ok, msg
    if numel >= 63:   # past saturation the reference is below 2^-30 |M|: the bound alone demands the near-zero there
        assert bool((x.abs() > 12 * cap).any()) and got[:, x.abs() > 12 * cap].abs().max().item() <= 3 * sr.EPS * M.abs().max().item()
