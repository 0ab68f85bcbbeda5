"""``kernels.cross_attention_jac_t`` (csrc/attention.hip, ``vivit_attention_cross_jac_t_f32``) against the fp64 reference under the
derived bounds of tests/attention_cross_refs.py, and the properties the rule promises: on a split packed projection with equal lengths
it has the bytes of the self-attention call; a sample with lengths has the bytes of the sample cut to its two lengths and run alone, and
exact zeros beyond; NaN and inf at dead positions reach nothing; a result that is not wanted is not computed and changes no byte of the
other; the bytes of a (v, n) slice depend on nothing around it; a misaligned operand gives the aligned call's bytes; finite results
for large logits; no ``Tq x Tk`` allocation; argument errors before any launch."""
import pytest
import torch

import attention_cross_refs as cr
from vivit_amd import kernels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [f"{i}-Tq{c[0]}-Tk{c[1]}-d{c[2]}-H{c[3]}-{c[4]}" for i, c in enumerate(cr.CASES)]


def run(M, q, kv, out, H, Hkv, scale, ql=None, kl=None, want=(True, True)):
    return kernels.cross_attention_jac_t(M.to(DEV), q.to(DEV), kv.to(DEV), out.to(DEV), H, scale, num_kv_heads=Hkv, query_lengths=ql,
                                         key_lengths=kl, want=want)


def check(G, M, q, kv, out, H, Hkv, scale, ql, kl, ref=None):
    Gq, bq, Gkv, bkv = ref or cr.rule(M, q, kv, out, H, Hkv, scale, ql, kl)
    dq, dk = cr.dead(q.shape[1], kv.shape[1], ql, kl, q.shape[0])
    half = kv.shape[-1] // 2
    for name, got, want, bound, dead in (("dQ", G[0].cpu(), Gq, bq, dq), ("dK", G[1].cpu()[..., :half], Gkv[..., :half], bkv[..., :half], dk),
                                         ("dV", G[1].cpu()[..., half:], Gkv[..., half:], bkv[..., half:], dk)):
        assert got.shape == want.shape and bool(torch.isfinite(got).all()), name
        err = (got.double() - want).abs()
        print(f"{name}: max error / bound = {(err / bound).max().item():.3g}, max error = {err.max().item():.3g}, "
              f"max |reference| = {want.abs().max().item():.3g}")
        ok, msg = cr.within(got, want, bound)
        assert ok, f"{name}: {msg}"
        assert bool((got[:, dead] == 0).all()), name


def poisoned(M, q, kv, out, dq, dk):
    """Copies with NaN and +-inf at the dead positions (plain data)."""
    M2, q2, kv2, o2 = M.clone(), q.clone(), kv.clone(), out.clone()
    M2[:, dq], o2[dq] = float("nan"), float("-inf")
    q2[dq], kv2[dk] = float("nan"), float("nan")
    q2[..., ::2][dq] = float("inf")
    kv2[..., 1::2][dk] = float("-inf")
    return M2, q2, kv2, o2


@pytest.mark.parametrize("i", range(len(cr.CASES)), ids=lambda i: IDS[i])
def test_cases(i):
    """Within the bounds and finite, exact zeros at the dead rows of both results; per sample the bytes of the sample cut to (Lq, Lk)
    and run alone without lengths; NaN / inf at the dead positions change no byte."""
    case = cr.CASES[i]
    Tq, Tk, d, H, Hkv, V, N, _, ql, kl = case
    M, q, kv, out, scale, He = cr.case_operands(case)
    G = run(M, q, kv, out, H, Hkv, scale, ql, kl)
    check(G, M, q, kv, out, H, He, scale, ql, kl, cr.case_rule(case))
    if ql is None and kl is None:
        return
    Gq, Gkv = G[0].cpu(), G[1].cpu()
    for n, (Lq, Lk) in enumerate(cr.live_lengths(Tq, Tk, ql, kl, N)):
        assert bool((Gq[:, n, Lq:] == 0).all()) and bool((Gkv[:, n, Lk:] == 0).all()), n
        if Lq > 0:
            aq, akv = run(M[:, n:n + 1, :Lq].contiguous(), q[n:n + 1, :Lq].contiguous(), kv[n:n + 1, :Lk].contiguous(),
                          out[n:n + 1, :Lq].contiguous(), H, Hkv, scale)
            assert tuple(aq.shape) == (V, 1, Lq, H * d) and tuple(akv.shape) == (V, 1, Lk, 2 * He * d)
            assert torch.equal(Gq[:, n, :Lq], aq[:, 0].cpu()) and torch.equal(Gkv[:, n, :Lk], akv[:, 0].cpu()), (n, Lq, Lk)
        else:
            assert bool((Gkv[:, n] == 0).all()), n       # (live keys that no query looks at)
    dq, dk = cr.dead(Tq, Tk, ql, kl, N)
    P = run(*poisoned(M, q, kv, out, dq, dk), H, Hkv, scale, ql, kl)
    assert torch.equal(P[0].cpu(), Gq) and torch.equal(P[1].cpu(), Gkv)


@pytest.mark.parametrize("lengths", [None, (70, 33, 0)], ids=["full", "lengths"])
@pytest.mark.parametrize("d,H,Hkv", [(20, 4, 2), (64, 4, 1)])
def test_a_split_packed_projection_has_the_bytes_of_the_self_attention_call(d, H, Hkv, lengths):
    V, N, T = 3, 3, 70
    M, qkv, out, scale = cr.mr.make_case(11 + d, V, N, T, H, Hkv, d, None, False, lengths, None)
    base = kernels.attention_jac_t(M.to(DEV), qkv.to(DEV), out.to(DEV), H, scale, False, num_kv_heads=Hkv, lengths=lengths, window=None)
    q, kv = qkv[..., :H * d].contiguous(), qkv[..., H * d:].contiguous()
    Gq, Gkv = run(M, q, kv, out, H, Hkv, scale, lengths, lengths)
    assert torch.equal(torch.cat((Gq, Gkv), -1), base)


@pytest.mark.parametrize("i", [8, 9, 14, 23], ids=lambda i: IDS[i])
def test_a_result_that_is_not_wanted_is_none_and_changes_no_byte_of_the_other(i):
    case = cr.CASES[i]
    Tq, Tk, d, H, Hkv, V, N, _, ql, kl = case
    M, q, kv, out, scale, He = cr.case_operands(case)
    Gq, Gkv = run(M, q, kv, out, H, Hkv, scale, ql, kl)
    only_q = run(M, q, kv, out, H, Hkv, scale, ql, kl, want=(True, False))
    only_kv = run(M, q, kv, out, H, Hkv, scale, ql, kl, want=(False, True))
    assert only_q[1] is None and only_kv[0] is None
    assert torch.equal(only_q[0], Gq) and torch.equal(only_kv[1], Gkv)


@pytest.mark.parametrize("d", [20, 64])
def test_bytes_do_not_depend_on_the_call_the_batch_or_the_chunk(d):
    V, N, Tq, Tk, H, Hkv = 3, 4, 70, 45, 4, 2
    ql, kl = (70, 33, 64, 1), (45, 32, 33, 45)
    M, q, kv, out, scale = cr.make_case(11 + d, V, N, Tq, Tk, H, Hkv, d, None, ql, kl)
    G1, G2 = run(M, q, kv, out, H, Hkv, scale, ql, kl), run(M, q, kv, out, H, Hkv, scale, ql, kl)
    assert torch.equal(G1[0], G2[0]) and torch.equal(G1[1], G2[1])
    # sample 2 with other lengths around it, and alone
    other = run(M, q, kv, out, H, Hkv, scale, (1, 70, 64, 0), (0, 45, 33, 1))
    assert torch.equal(G1[0][:, 2], other[0][:, 2]) and torch.equal(G1[1][:, 2], other[1][:, 2])
    alone = run(M[1:2, 2:3].contiguous(), q[2:3].contiguous(), kv[2:3].contiguous(), out[2:3].contiguous(), H, Hkv, scale, ql[2:3], kl[2:3])
    assert torch.equal(G1[0][1, 2], alone[0][0, 0]) and torch.equal(G1[1][1, 2], alone[1][0, 0])
    # rows of a later chunk, of a chunk's last place and of a ragged last chunk: chunks 4, 4, 1 (d = 20) and 2, 2, 1 (d = 64)
    V, rows = (9, (3, 4, 8)) if d == 20 else (5, (1, 2, 4))
    assert V == 2 * cr.chunk(d) + 1
    M, q, kv, out, scale = cr.make_case(13 + d, V, N, Tq, Tk, H, Hkv, d, None, ql, kl)
    G = run(M, q, kv, out, H, Hkv, scale, ql, kl)
    check(G, M, q, kv, out, H, Hkv, scale, ql, kl)
    for v in rows:
        alone = run(M[v:v + 1].contiguous(), q, kv, out, H, Hkv, scale, ql, kl)
        assert torch.equal(G[0][v], alone[0][0]) and torch.equal(G[1][v], alone[1][0]), v


def test_large_logits():
    """q and k scaled until the logits span about +-150 and beyond, with lengths on both sides."""
    V, N, Tq, Tk, H, Hkv, d = 3, 2, 40, 50, 4, 2, 20
    ql, kl = (40, 33), (50, 31)
    M, q, kv, out, scale = cr.make_case(7, V, N, Tq, Tk, H, Hkv, d, None, ql, kl, qk_gain=8.0)
    S = cr.logits(q, kv, H, Hkv, scale)
    assert S.max().item() > 150 and S.min().item() < -150
    check(run(M, q, kv, out, H, Hkv, scale, ql, kl), M, q, kv, out, H, Hkv, scale, ql, kl)


@pytest.mark.parametrize("which", ["M", "q", "kv"])
@pytest.mark.parametrize("d", [4, 20, 64, 128])
def test_operand_four_bytes_off_a_16_byte_boundary(d, which):
    V, N, Tq, Tk, H, Hkv = 3, 2, 40, 35, 3, 1
    ql, kl = (40, 31), (33, 35)
    M, q, kv, out, scale = cr.make_case(17 + d, V, N, Tq, Tk, H, Hkv, d, None, ql, kl)
    ops = {"M": M.to(DEV), "q": q.to(DEV), "kv": kv.to(DEV)}
    assert all(t.data_ptr() % 16 == 0 for t in ops.values())
    call = lambda: kernels.cross_attention_jac_t(ops["M"], ops["q"], ops["kv"], out.to(DEV), H, scale, num_kv_heads=Hkv,   # noqa: E731
                                                 query_lengths=ql, key_lengths=kl)
    aligned = call()
    ops[which] = cr.misaligned(ops[which])
    assert ops[which].data_ptr() % 16 == 4
    G = call()
    check(G, M, q, kv, out, H, Hkv, scale, ql, kl)
    assert torch.equal(G[0], aligned[0]) and torch.equal(G[1], aligned[1])


def test_no_tq_by_tk_allocation():
    V, N, Tq, Tk, H, Hkv, d = 4, 2, 64, 256, 4, 1, 16
    ql, kl = (64, 40), (256, 100)
    M, q, kv, out, scale = cr.make_case(3, V, N, Tq, Tk, H, Hkv, d, None, ql, kl)
    Md, qd, kvd, od = M.to(DEV), q.to(DEV), kv.to(DEV), out.to(DEV)
    qld, kld = torch.tensor(ql, dtype=torch.int32, device=DEV), torch.tensor(kl, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    G = kernels.cross_attention_jac_t(Md, qd, kvd, od, H, scale, num_kv_heads=Hkv, query_lengths=qld, key_lengths=kld)
    torch.cuda.synchronize()
    assert tuple(G[0].shape) == (V, N, Tq, H * d) and tuple(G[1].shape) == (V, N, Tk, 2 * Hkv * d)
    extra = torch.cuda.max_memory_allocated() - before - (G[0].numel() + G[1].numel()) * 4
    assert extra < N * Tq * Tk, extra                                      # not even one byte per (n, i, j)
    check(G, M, q, kv, out, H, Hkv, scale, ql, kl)


def test_argument_errors_come_before_any_launch():
    z = lambda *s: torch.zeros(*s, device=DEV)   # noqa: E731
    args = (z(1, 2, 3, 16), z(2, 3, 16), z(2, 5, 16), z(2, 3, 16), 4, 1.0)
    for name in ("query_lengths", "key_lengths"):
        for lengths in ([3], [3, 3, 3], [[3, 3]], torch.tensor(3)):
            with pytest.raises(ValueError, match=name + " must be"):
                kernels.cross_attention_jac_t(*args, num_kv_heads=2, **{name: lengths})
        for lengths in ([3.0, 2.0], torch.ones(2, device=DEV), torch.ones(2, dtype=torch.bool)):
            with pytest.raises(ValueError, match=name + " must be integers"):
                kernels.cross_attention_jac_t(*args, num_kv_heads=2, **{name: lengths})
    with pytest.raises(ValueError, match="want must name"):
        kernels.cross_attention_jac_t(*args, num_kv_heads=2, want=(False, False))
    with pytest.raises(ValueError, match="positive multiple"):
        kernels.cross_attention_jac_t(*args, num_kv_heads=3)
    with pytest.raises(ValueError, match=r"kv must be \[2, Tk, 2 \* 2 \* 4\]"):
        kernels.cross_attention_jac_t(z(1, 2, 3, 16), z(2, 3, 16), z(2, 5, 32), z(2, 3, 16), 4, 1.0, num_kv_heads=2)
    with pytest.raises(ValueError, match=r"q must be \[N, Tq, 4 \* d\]"):
        kernels.cross_attention_jac_t(z(1, 2, 3, 18), z(2, 3, 18), z(2, 5, 16), z(2, 3, 18), 4, 1.0, num_kv_heads=2)
    with pytest.raises(ValueError, match="out must be"):
        kernels.cross_attention_jac_t(z(1, 2, 3, 16), z(2, 3, 16), z(2, 5, 16), z(2, 4, 16), 4, 1.0, num_kv_heads=2)
    with pytest.raises(ValueError, match=r"M must be \[V, 2, 3, 16\]"):
        kernels.cross_attention_jac_t(z(1, 2, 4, 16), z(2, 3, 16), z(2, 5, 16), z(2, 3, 16), 4, 1.0, num_kv_heads=2)
    with pytest.raises(ValueError, match="empty operands"):
        kernels.cross_attention_jac_t(z(1, 2, 3, 16), z(2, 3, 16), z(2, 0, 16), z(2, 3, 16), 4, 1.0, num_kv_heads=2)
    with pytest.raises(RuntimeError, match="HIP-device tensors"):
        kernels.cross_attention_jac_t(torch.zeros(1, 2, 3, 16), *args[1:], num_kv_heads=2)
