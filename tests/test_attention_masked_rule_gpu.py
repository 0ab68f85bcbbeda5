"""``kernels.attention_jac_t(..., lengths=, window=)`` (csrc/attention.hip, ``vivit_attention_masked_jac_t_f32``) against the fp64
reference under the derived bounds of tests/attention_masked_refs.py, and the properties the rule promises: a sample with lengths has
the bytes of the sample cut to its length and run alone, and exact zeros beyond; NaN and inf at dead positions reach nothing; no
lengths, full lengths and a window of ``T`` or more are the unmasked call byte for byte; ``num_kv_heads == num_heads`` is the
multi-head call; exact zeros where a causal window cuts; the bytes of a (v, n) slice depend on nothing around it; finite results for
large logits; no ``T x T`` allocation; argument errors before any launch."""
import pytest
import torch

import attention_masked_refs as mr
from vivit_amd import kernels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [f"{i}-T{c[0]}-d{c[1]}-H{c[2]}-{c[3]}-W{c[9]}-{'c' if c[6] else 'f'}" for i, c in enumerate(mr.CASES)]


def run(M, qkv, out, H, Hkv, scale, causal, lengths=None, window=None):
    return kernels.attention_jac_t(M.to(DEV), qkv.to(DEV), out.to(DEV), H, scale, causal, num_kv_heads=Hkv, lengths=lengths, window=window)


def check(G, M, qkv, out, H, Hkv, scale, causal, lengths, window):
    ref, bound = mr.rule(M, qkv, out, H, Hkv, scale, causal, lengths, window)
    got = G.cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    d = M.shape[-1] // H
    for name, sl in (("dQ", slice(0, H * d)), ("dK", slice(H * d, (H + Hkv) * d)), ("dV", slice((H + Hkv) * d, (H + 2 * Hkv) * d))):
        err = (got[..., sl].double() - ref[..., sl]).abs()
        print(f"{name}: max error / bound = {(err / bound[..., sl]).max().item():.3g}, max error = {err.max().item():.3g}, "
              f"max |reference| = {ref[..., sl].abs().max().item():.3g}")
    ok, msg = mr.within(got, ref, bound)
    assert ok, msg
    dead = mr.dead(M.shape[2], lengths, M.shape[1])
    assert bool((got[:, dead] == 0).all())


def poisoned(M, qkv, out, lengths):
    """Copies with NaN and +-inf at the dead positions (plain data)."""
    dead = mr.dead(M.shape[2], lengths, M.shape[1])
    M2, q2, o2 = M.clone(), qkv.clone(), out.clone()
    M2[:, dead], o2[dead] = float("nan"), float("-inf")
    q2[dead] = float("nan")
    q2[..., ::2][dead] = float("inf")
    return M2, q2, o2


@pytest.mark.parametrize("i", range(len(mr.CASES)), ids=lambda i: IDS[i])
def test_cases(i):
    """Within the bounds and finite; per sample the bytes of the truncated sample run alone by the unmasked call (the windowed one
    where the case has a window) and exact zeros beyond; NaN / inf at the dead positions change no byte."""
    T, d, H, Hkv, V, N, causal, _, lengths, window = mr.CASES[i]
    M, qkv, out, scale, He = mr.case_operands(mr.CASES[i])
    G = run(M, qkv, out, H, Hkv, scale, causal, lengths, window)
    check(G, M, qkv, out, H, He, scale, causal, lengths, window)
    if lengths is None:
        return
    G = G.cpu()
    for n, L in enumerate(lengths):
        assert bool((G[:, n, L:] == 0).all()), n
        if L > 0:
            alone = run(M[:, n:n + 1, :L].contiguous(), qkv[n:n + 1, :L].contiguous(), out[n:n + 1, :L].contiguous(), H, Hkv, scale, causal,
                        None, window)
            assert tuple(alone.shape) == (V, 1, L, G.shape[-1])
            assert torch.equal(G[:, n, :L], alone[:, 0].cpu()), (n, L)
    M2, q2, o2 = poisoned(M, qkv, out, lengths)
    assert torch.equal(run(M2, q2, o2, H, Hkv, scale, causal, lengths, window).cpu(), G)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d,Hkv", [(20, None), (64, 2)])
def test_identities(d, Hkv, causal):
    """No lengths and no window is the existing call; all lengths ``T`` and a window of ``T`` or more give its bytes."""
    V, N, T, H = 3, 3, 70, 4
    M, qkv, out, scale = mr.gr.make_case(11 + d, V, N, T, H, H if Hkv is None else Hkv, d, None, causal)
    base = kernels.attention_jac_t(M.to(DEV), qkv.to(DEV), out.to(DEV), H, scale, causal, num_kv_heads=Hkv)
    assert torch.equal(run(M, qkv, out, H, Hkv, scale, causal, None, None), base)
    assert torch.equal(run(M, qkv, out, H, Hkv, scale, causal, [T] * N, None), base)
    assert torch.equal(run(M, qkv, out, H, Hkv, scale, causal, torch.full((N,), T, dtype=torch.int64, device=DEV), T), base)
    assert torch.equal(run(M, qkv, out, H, Hkv, scale, causal, torch.full((N,), T + 9), None), base)   # (a device would clamp: so does this)
    for window in (T, T + 5, 2 ** 31 - 1, 2 ** 40):
        assert torch.equal(run(M, qkv, out, H, Hkv, scale, causal, None, window), base), window


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [20, 64])
def test_equal_head_counts_are_the_multi_head_call(d, causal):
    V, N, T, H = 3, 3, 70, 2
    lengths, window = (70, 33, 0), 34
    M, qkv, out, scale = mr.make_case(13 + d, V, N, T, H, H, d, None, causal, lengths, window)
    assert torch.equal(run(M, qkv, out, H, None, scale, causal, lengths, window), run(M, qkv, out, H, H, scale, causal, lengths, window))


@pytest.mark.parametrize("a,b,W", [(40, 50, 8), (32, 64, 32), (33, 65, 33), (64, 70, 34), (5, 6, 1), (64, 96, 65), (31, 33, 2)])
def test_causal_window_structure(a, b, W):
    """Causal with window W: key j is seen by the queries j .. j + W - 1.  A factor that is nonzero only at the query rows [a, b) leaves
    dK and dV exactly zero at the keys j <= a - W and j >= b, and nonzero at every key in between (a, b and W on and off the block
    boundaries)."""
    V, N, T, H, Hkv, d = 3, 2, 100, 4, 2, 20
    M, qkv, out, scale = mr.make_case(5 + W, V, N, T, H, Hkv, d, None, True, None, W)
    M[:, :, :a] = 0.0
    M[:, :, b:] = 0.0
    G = run(M, qkv, out, H, Hkv, scale, True, None, W).cpu()
    check(G, M, qkv, out, H, Hkv, scale, True, None, W)
    kv = G[..., H * d:]
    lo = max(a - W + 1, 0)
    assert bool((kv[:, :, :lo] == 0).all()) and bool((kv[:, :, b:] == 0).all())
    assert bool((kv[:, :, lo:b].abs().amax((0, 1, 3)) > 0).all())
    # dQ: a query hears back only through its own dO, so the rows outside [a, b) are exactly zero as well
    dq = G[..., :H * d]
    assert bool((dq[:, :, :a] == 0).all()) and bool((dq[:, :, b:] == 0).all()) and bool((dq[:, :, a:b].abs().amax((0, 1, 3)) > 0).all())


@pytest.mark.parametrize("d", [20, 64])
def test_bytes_do_not_depend_on_the_call_the_batch_or_the_chunk(d):
    V, N, T, H, Hkv, W = 3, 4, 70, 4, 2, 33
    lengths = (70, 33, 64, 1)
    M, qkv, out, scale = mr.make_case(11 + d, V, N, T, H, Hkv, d, None, True, lengths, W)
    G1, G2 = run(M, qkv, out, H, Hkv, scale, True, lengths, W), run(M, qkv, out, H, Hkv, scale, True, lengths, W)
    assert torch.equal(G1, G2)
    # sample 2 with other lengths around it, and alone
    other = run(M, qkv, out, H, Hkv, scale, True, (1, 70, 64, 0), W)
    assert torch.equal(G1[:, 2], other[:, 2])
    alone = run(M[1:2, 2:3].contiguous(), qkv[2:3].contiguous(), out[2:3].contiguous(), H, Hkv, scale, True, lengths[2:3], W)
    assert torch.equal(G1[1, 2], alone[0, 0])
    # rows of a later chunk, of a chunk's last place and of a ragged last chunk: chunks 4, 4, 1 (d = 20) and 2, 2, 1 (d = 64)
    V, rows = (9, (3, 4, 8)) if d == 20 else (5, (1, 2, 4))
    assert V == 2 * mr.chunk(d) + 1
    M, qkv, out, scale = mr.make_case(13 + d, V, N, T, H, Hkv, d, None, True, lengths, W)
    G = run(M, qkv, out, H, Hkv, scale, True, lengths, W)
    check(G, M, qkv, out, H, Hkv, scale, True, lengths, W)
    for v in rows:
        alone = run(M[v:v + 1].contiguous(), qkv, out, H, Hkv, scale, True, lengths, W)
        assert torch.equal(G[v], alone[0]), v


@pytest.mark.parametrize("causal", [False, True])
def test_large_logits(causal):
    """q and k scaled until the logits span about +-150 and beyond, with a window and lengths."""
    V, N, T, H, Hkv, d = 3, 2, 40, 4, 2, 20
    lengths, W = (40, 33), 9
    M, qkv, out, scale = mr.make_case(7, V, N, T, H, Hkv, d, None, causal, lengths, W, qk_gain=8.0)
    S = mr.gr.logits(qkv, H, Hkv, scale)
    assert S.max().item() > 150 and S.min().item() < -150
    check(run(M, qkv, out, H, Hkv, scale, causal, lengths, W), M, qkv, out, H, Hkv, scale, causal, lengths, W)


@pytest.mark.parametrize("which", ["M", "qkv"])
@pytest.mark.parametrize("d", [4, 20, 64, 128])
def test_operand_four_bytes_off_a_16_byte_boundary(d, which):
    V, N, T, H, Hkv, W = 3, 2, 40, 3, 1, 33
    lengths = (40, 31)
    M, qkv, out, scale = mr.make_case(17 + d, V, N, T, H, Hkv, d, None, True, lengths, W)
    Md, qd, od = M.to(DEV), qkv.to(DEV), out.to(DEV)
    assert Md.data_ptr() % 16 == 0 and qd.data_ptr() % 16 == 0
    aligned = kernels.attention_jac_t(Md, qd, od, H, scale, True, num_kv_heads=Hkv, lengths=lengths, window=W)
    if which == "M":
        Md = mr.misaligned(Md)
    else:
        qd = mr.misaligned(qd)
    assert (Md if which == "M" else qd).data_ptr() % 16 == 4
    G = kernels.attention_jac_t(Md, qd, od, H, scale, True, num_kv_heads=Hkv, lengths=lengths, window=W)
    check(G, M, qkv, out, H, Hkv, scale, True, lengths, W)
    assert torch.equal(G, aligned)


def test_no_t_by_t_allocation():
    V, N, T, H, Hkv, d = 4, 2, 256, 4, 1, 16
    lengths, W = torch.tensor([256, 100], dtype=torch.int32, device=DEV), 40
    M, qkv, out, scale = mr.make_case(3, V, N, T, H, Hkv, d, None, False, (256, 100), W)
    Md, qd, od = M.to(DEV), qkv.to(DEV), out.to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    G = kernels.attention_jac_t(Md, qd, od, H, scale, False, num_kv_heads=Hkv, lengths=lengths, window=W)
    torch.cuda.synchronize()
    assert tuple(G.shape) == (V, N, T, (H + 2 * Hkv) * d)
    extra = torch.cuda.max_memory_allocated() - before - G.numel() * 4
    assert extra < N * T * T, extra                                        # not even one byte per (n, i, j)
    check(G, M, qkv, out, H, Hkv, scale, False, (256, 100), W)


def test_argument_errors_come_before_any_launch():
    z = lambda *s: torch.zeros(*s, device=DEV)   # noqa: E731
    args = (z(1, 2, 3, 16), z(2, 3, 32), z(2, 3, 16), 4, 1.0, False)
    for lengths in ([3], [3, 3, 3], [[3, 3]], torch.tensor(3)):
        with pytest.raises(ValueError, match="lengths must be"):
            kernels.attention_jac_t(*args, num_kv_heads=2, lengths=lengths)
    for lengths in ([3.0, 2.0], torch.ones(2, device=DEV), torch.ones(2, dtype=torch.bool)):
        with pytest.raises(ValueError, match="lengths must be integers"):
            kernels.attention_jac_t(*args, num_kv_heads=2, lengths=lengths)
    for window in (0, -3, 1.5):
        with pytest.raises(ValueError, match="window must be"):
            kernels.attention_jac_t(*args, num_kv_heads=2, window=window)
    with pytest.raises(ValueError, match="out must be"):                  # the older checks still come
        kernels.attention_jac_t(z(1, 2, 3, 16), z(2, 3, 32), z(2, 3, 32), 4, 1.0, False, num_kv_heads=2, lengths=[3, 3], window=2)
