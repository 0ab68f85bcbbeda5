"""``kernels.attention_jac_t(..., num_kv_heads=Hkv)`` (csrc/attention.hip, ``vivit_attention_gqa_jac_t_f32``) at its edge shapes against
the fp64 reference under the derived bounds of tests/attention_gqa_refs.py, and the properties the rule promises: ``Hkv == H`` is the
multi-head kernel byte for byte, equal bytes from call to call and for a (v, n) slice whatever the batch around it, a key / value
head hears from the query heads of its own group and from no other, exact zeros where the causal mask cuts, finite results for large
logits, no ``T x T`` allocation."""
import pytest
import torch

import attention_gqa_refs as gr
from vivit_amd import kernels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def run(M, qkv, out, H, Hkv, scale, causal):
    return kernels.attention_jac_t(M.to(DEV), qkv.to(DEV), out.to(DEV), H, scale, causal, num_kv_heads=Hkv)


def check(G, M, qkv, out, H, Hkv, scale, causal):
    ref, bound = gr.rule(M, qkv, out, H, Hkv, scale, causal)
    got = G.cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    d = M.shape[-1] // H
    for name, sl in (("dQ", slice(0, H * d)), ("dK", slice(H * d, (H + Hkv) * d)), ("dV", slice((H + Hkv) * d, (H + 2 * Hkv) * d))):
        err = (got[..., sl].double() - ref[..., sl]).abs()
        print(f"{name}: max error / bound = {(err / bound[..., sl]).max().item():.3g}, max error = {err.max().item():.3g}, "
              f"max |reference| = {ref[..., sl].abs().max().item():.3g}")
    ok, msg = gr.within(got, ref, bound)
    assert ok, msg


@pytest.mark.parametrize("T,d,H,Hkv,V,N,causal,scale", gr.CASES)
def test_edge_shapes(T, d, H, Hkv, V, N, causal, scale):
    M, qkv, out, scale = gr.make_case(1000 * T + d + H, V, N, T, H, Hkv, d, scale, causal)
    G = run(M, qkv, out, H, Hkv, scale, causal)
    check(G, M, qkv, out, H, Hkv, scale, causal)
    if scale == 0.0:
        assert bool((G[..., :(H + Hkv) * d] == 0).all())                              # dQ and dK
        assert bool((G[..., (H + Hkv) * d:].abs().amax((0, 2, 3)) > 0).all())         # dV does not depend on the scale


@pytest.mark.parametrize("d", [20, 64])
def test_equal_head_counts_are_the_multi_head_kernel(d):
    """``num_kv_heads == num_heads`` and no ``num_kv_heads``: one kernel, one order of summation, the same bytes."""
    V, N, T, H = 3, 3, 40, 2
    M, qkv, out, scale = gr.ar.make_case(11 + d, V, N, T, H, d, None, True)
    old = kernels.attention_jac_t(M.to(DEV), qkv.to(DEV), out.to(DEV), H, scale, True)
    new = run(M, qkv, out, H, H, scale, True)
    assert torch.equal(old, new)
    check(new, M, qkv, out, H, H, scale, True)


@pytest.mark.parametrize("d", [20, 64])
def test_bytes_do_not_depend_on_the_call_or_the_batch(d):
    V, N, T, H, Hkv = 3, 3, 40, 4, 2
    M, qkv, out, scale = gr.make_case(11 + d, V, N, T, H, Hkv, d, None, True)
    G1, G2 = run(M, qkv, out, H, Hkv, scale, True), run(M, qkv, out, H, Hkv, scale, True)
    assert torch.equal(G1, G2)
    alone = run(M[1:2, 2:3].contiguous(), qkv[2:3].contiguous(), out[2:3].contiguous(), H, Hkv, scale, True)
    assert torch.equal(G1[1, 2], alone[0, 0])
    # rows of a later chunk, of a chunk's last place and of a ragged last chunk: chunks 4, 4, 1 (d = 20) and 2, 2, 1 (d = 64)
    V, rows = (9, (3, 4, 8)) if d == 20 else (5, (1, 2, 4))
    assert V == 2 * gr.chunk(d) + 1
    M, qkv, out, scale = gr.make_case(13 + d, V, N, T, H, Hkv, d, None, True)
    G = run(M, qkv, out, H, Hkv, scale, True)
    check(G, M, qkv, out, H, Hkv, scale, True)
    for v in rows:
        alone = run(M[v:v + 1].contiguous(), qkv, out, H, Hkv, scale, True)
        assert torch.equal(G[v], alone[0]), v


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [20, 64])
def test_group_isolation(d, causal):
    """H = 6 query heads in Hkv = 3 groups of two.  A factor that is zero on both heads of group 1 leaves dK and dV of key / value head
    1 and dQ of those heads exactly zero and every other head nonzero; a factor that is zero on ONE head of a group leaves the group's
    dK and dV byte-equal to the multi-head kernel run on the other head alone (H = 1 with the group's K and V): the owner's walk
    starts and ends at the right heads, and adds nothing else."""
    V, N, T, H, Hkv = 3, 2, 40, 6, 3
    M, qkv, out, scale = gr.make_case(23 + d, V, N, T, H, Hkv, d, None, causal)
    q0, k0, v0 = 0, H * d, (H + Hkv) * d
    Mz = M.clone()
    Mz[..., 2 * d:4 * d] = 0.0
    G = run(Mz, qkv, out, H, Hkv, scale, causal).cpu()
    check(G, Mz, qkv, out, H, Hkv, scale, causal)
    assert bool((G[..., k0 + d:k0 + 2 * d] == 0).all()) and bool((G[..., v0 + d:v0 + 2 * d] == 0).all())
    assert bool((G[..., q0 + 2 * d:q0 + 4 * d] == 0).all())
    for g in (0, 2):
        assert bool((G[..., k0 + g * d:k0 + (g + 1) * d].abs().amax((0, 2, 3)) > 0).all())
        assert bool((G[..., v0 + g * d:v0 + (g + 1) * d].abs().amax((0, 2, 3)) > 0).all())
        for h in (2 * g, 2 * g + 1):
            assert bool((G[..., q0 + h * d:q0 + (h + 1) * d].abs().amax((0, 2, 3)) > 0).all())
    for silent, other in ((2, 3), (3, 2), (4, 5), (1, 0)):
        g = other // 2
        Mz = M.clone()
        Mz[..., silent * d:(silent + 1) * d] = 0.0
        G = run(Mz, qkv, out, H, Hkv, scale, causal).cpu()
        col = lambda t, h: t[..., h * d:(h + 1) * d]   # noqa: E731
        one = torch.cat((col(qkv, other), col(qkv[..., k0:], g), col(qkv[..., v0:], g)), -1).contiguous()
        single = kernels.attention_jac_t(col(M, other).contiguous().to(DEV), one.to(DEV), col(out, other).contiguous().to(DEV), 1, scale,
                                         causal).cpu()
        assert torch.equal(col(G, other), single[..., :d])                       # dQ of the speaking head
        assert torch.equal(col(G[..., k0:], g), single[..., d:2 * d]), (silent, other)
        assert torch.equal(col(G[..., v0:], g), single[..., 2 * d:]), (silent, other)
        assert bool((col(G, silent) == 0).all())


@pytest.mark.parametrize("j0", [19, 32])
def test_causal_structure(j0):
    """With the causal mask a key j hears only from the queries i >= j, of every head of its group: a factor that is zero at the rows
    >= j0 leaves dK[j0:] and dV[j0:] exactly zero (and must leave something in the rows before)."""
    V, N, T, H, Hkv, d = 3, 2, 40, 4, 2, 20
    M, qkv, out, scale = gr.make_case(5, V, N, T, H, Hkv, d, None, True)
    M[:, :, j0:] = 0.0
    G = run(M, qkv, out, H, Hkv, scale, True).cpu()
    E = H * d
    assert bool((G[:, :, j0:, E:] == 0).all())
    assert bool((G[:, :, :j0, E:].abs().amax((0, 1, 3)) > 0).all())
    check(G, M, qkv, out, H, Hkv, scale, True)


@pytest.mark.parametrize("causal", [False, True])
def test_large_logits(causal):
    """q and k scaled until the logits span about +-200: exp of anything but a max- or lse-subtracted argument overflows."""
    V, N, T, H, Hkv, d = 3, 2, 33, 4, 2, 20
    M, qkv, out, scale = gr.make_case(7, V, N, T, H, Hkv, d, None, causal, qk_gain=8.0)
    S = gr.logits(qkv, H, Hkv, scale)
    assert S.max().item() > 150 and S.min().item() < -150
    check(run(M, qkv, out, H, Hkv, scale, causal), M, qkv, out, H, Hkv, scale, causal)


@pytest.mark.parametrize("which", ["M", "qkv"])
@pytest.mark.parametrize("d", [4, 20, 64, 128])
def test_operand_four_bytes_off_a_16_byte_boundary(d, which):
    """d % 4 == 0 with an operand that is not 16-byte aligned: the scalar load body of every instance.  The loads change, the
    arithmetic does not: the bytes are those of the aligned call."""
    V, N, T, H, Hkv = 3, 1, 33, 3, 1
    M, qkv, out, scale = gr.make_case(17 + d, V, N, T, H, Hkv, d, None, True)
    Md, qd, od = M.to(DEV), qkv.to(DEV), out.to(DEV)
    assert Md.data_ptr() % 16 == 0 and qd.data_ptr() % 16 == 0
    aligned = kernels.attention_jac_t(Md, qd, od, H, scale, True, num_kv_heads=Hkv)
    if which == "M":
        Md = gr.misaligned(Md)
    else:
        qd = gr.misaligned(qd)
    assert (Md if which == "M" else qd).data_ptr() % 16 == 4
    G = kernels.attention_jac_t(Md, qd, od, H, scale, True, num_kv_heads=Hkv)
    check(G, M, qkv, out, H, Hkv, scale, True)
    assert torch.equal(G, aligned)


def test_no_t_by_t_allocation():
    V, N, T, H, Hkv, d = 4, 2, 256, 4, 1, 16
    M, qkv, out, scale = gr.make_case(3, V, N, T, H, Hkv, d)
    M, qkv, out = M.to(DEV), qkv.to(DEV), out.to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    G = kernels.attention_jac_t(M, qkv, out, H, scale, False, num_kv_heads=Hkv)
    torch.cuda.synchronize()
    assert tuple(G.shape) == (V, N, T, (H + 2 * Hkv) * d) and G.shape[-1] != 3 * H * d
    extra = torch.cuda.max_memory_allocated() - before - G.numel() * 4
    assert extra < V * N * H * T * T * 4, extra
    check(G, M.cpu(), qkv.cpu(), out.cpu(), H, Hkv, scale, False)


def test_shape_errors_come_before_any_launch():
    z = lambda *s: torch.zeros(*s, device=DEV)   # noqa: E731
    with pytest.raises(ValueError, match="multiple of num_kv_heads"):
        kernels.attention_jac_t(z(1, 1, 3, 16), z(1, 3, 40), z(1, 3, 16), 4, 1.0, False, num_kv_heads=3)
    with pytest.raises(ValueError, match="num_kv_heads"):
        kernels.attention_jac_t(z(1, 1, 3, 16), z(1, 3, 24), z(1, 3, 16), 4, 1.0, False, num_kv_heads=0)
    with pytest.raises(ValueError, match=r"\(4 \+ 2 \* 2\) \* d"):
        kernels.attention_jac_t(z(1, 1, 3, 16), z(1, 3, 36), z(1, 3, 16), 4, 1.0, False, num_kv_heads=2)
    with pytest.raises(ValueError, match="out must be"):
        kernels.attention_jac_t(z(1, 1, 3, 16), z(1, 3, 32), z(1, 3, 32), 4, 1.0, False, num_kv_heads=2)
    with pytest.raises(ValueError, match="M must be"):
        kernels.attention_jac_t(z(1, 1, 3, 32), z(1, 3, 32), z(1, 3, 16), 4, 1.0, False, num_kv_heads=2)
    with pytest.raises(ValueError, match="3 \\* 4 \\* d"):                      # without the argument: the old check and its message
        kernels.attention_jac_t(z(1, 1, 3, 16), z(1, 3, 32), z(1, 3, 16), 4, 1.0, False)
