"""``kernels.attention_jac_t`` (csrc/attention.hip) at its edge shapes against the fp64 reference under the derived bounds of
tests/attention_refs.py, and the properties the rule promises: finite results for large logits, equal bytes from call to call and
for a (v, n) slice whatever the batch around it, exact zeros where the causal mask cuts, no ``T x T`` allocation."""
import pytest
import torch

import attention_refs as ar
from vivit_amd import _lib, kernels
from vivit_amd.backend import ScaledDotProductAttention
from vivit_amd.backend.extensions import _jac_t_mat_prod

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TB, CASES = ar.TB, ar.CASES   # the list and its rule: tests/attention_refs.py


def run(M, qkv, out, H, scale, causal):
    return kernels.attention_jac_t(M.to(DEV), qkv.to(DEV), out.to(DEV), H, scale, causal)


def check(G, M, qkv, out, H, scale, causal):
    ref, bound = ar.rule(M, qkv, out, H, scale, causal)
    got = G.cpu()
    assert bool(torch.isfinite(got).all())
    E = M.shape[-1]
    for name, sl in (("dQ", slice(0, E)), ("dK", slice(E, 2 * E)), ("dV", slice(2 * E, 3 * E))):
        err = (got[..., sl].double() - ref[..., sl]).abs()
        print(f"{name}: max error / bound = {(err / bound[..., sl]).max().item():.3g}, max error = {err.max().item():.3g}, "
              f"max |reference| = {ref[..., sl].abs().max().item():.3g}")
    ok, msg = ar.within(got, ref, bound)
    assert ok, msg


@pytest.mark.parametrize("T,d,H,V,N,causal,scale", CASES)
def test_edge_shapes(T, d, H, V, N, causal, scale):
    M, qkv, out, scale = ar.make_case(1000 * T + d, V, N, T, H, d, scale, causal)
    G = run(M, qkv, out, H, scale, causal)
    check(G, M, qkv, out, H, scale, causal)
    if scale == 0.0:
        assert bool((G[..., :2 * H * d] == 0).all())                     # dQ and dK
        assert bool((G[..., 2 * H * d:].abs().amax((0, 2, 3)) > 0).all())    # dV does not depend on the scale


@pytest.mark.parametrize("causal", [False, True])
def test_large_logits(causal):
    """q and k scaled until the logits span about +-200: exp of anything but a max- or lse-subtracted argument overflows."""
    V, N, T, H, d = 3, 2, 33, 2, 20
    M, qkv, out, scale = ar.make_case(7, V, N, T, H, d, None, causal, qk_gain=8.0)
    S = ar.logits(qkv, H, scale)
    assert S.max().item() > 150 and S.min().item() < -150
    check(run(M, qkv, out, H, scale, causal), M, qkv, out, H, scale, causal)


@pytest.mark.parametrize("d", [20, 64])
def test_bytes_do_not_depend_on_the_call_or_the_batch(d):
    V, N, T, H = 3, 3, 40, 2
    M, qkv, out, scale = ar.make_case(11 + d, V, N, T, H, d, None, True)
    G1, G2 = run(M, qkv, out, H, scale, True), run(M, qkv, out, H, scale, True)
    assert torch.equal(G1, G2)
    alone = run(M[1:2, 2:3].contiguous(), qkv[2:3].contiguous(), out[2:3].contiguous(), H, scale, True)
    assert torch.equal(G1[1, 2], alone[0, 0])
    # rows of a later chunk, of a chunk's last place and of a ragged last chunk: chunks 4, 4, 1 (d = 20) and 2, 2, 1 (d = 64)
    V, rows = (9, (3, 4, 8)) if d == 20 else (5, (1, 2, 4))
    assert V == 2 * ar.chunk(d) + 1
    M, qkv, out, scale = ar.make_case(13 + d, V, N, T, H, d, None, True)
    G = run(M, qkv, out, H, scale, True)
    check(G, M, qkv, out, H, scale, True)
    for v in rows:
        alone = run(M[v:v + 1].contiguous(), qkv, out, H, scale, True)
        assert torch.equal(G[v], alone[0]), v


@pytest.mark.parametrize("which", ["M", "qkv"])
@pytest.mark.parametrize("d", [4, 20, 64, 128])
def test_operand_four_bytes_off_a_16_byte_boundary(d, which):
    """d % 4 == 0 with an operand that is not 16-byte aligned: the scalar load body of every instance.  The loads change, the
    arithmetic does not: the bytes are those of the aligned call."""
    V, N, T, H = 3, 1, 33, 1
    M, qkv, out, scale = ar.make_case(17 + d, V, N, T, H, d, None, True)
    Md, qd, od = M.to(DEV), qkv.to(DEV), out.to(DEV)
    assert Md.data_ptr() % 16 == 0 and qd.data_ptr() % 16 == 0
    aligned = kernels.attention_jac_t(Md, qd, od, H, scale, True)
    if which == "M":
        Md = ar.misaligned(Md)
        assert Md.data_ptr() % 16 == 4 and Md.is_contiguous()
    else:
        qd = ar.misaligned(qd)
        assert qd.data_ptr() % 16 == 4 and qd.is_contiguous()
    G = kernels.attention_jac_t(Md, qd, od, H, scale, True)
    check(G, M, qkv, out, H, scale, True)
    assert torch.equal(G, aligned)


@pytest.mark.parametrize("j0", [19, 32])
def test_causal_structure(j0):
    """With the causal mask a key j hears only from the queries i >= j: a factor that is zero at the rows >= j0 leaves dK[j0:] and
    dV[j0:] exactly zero (and must leave something in the rows before)."""
    V, N, T, H, d = 3, 2, 40, 3, 20
    M, qkv, out, scale = ar.make_case(5, V, N, T, H, d, None, True)
    M[:, :, j0:] = 0.0
    G = run(M, qkv, out, H, scale, True).cpu()
    E = H * d
    assert bool((G[:, :, j0:, E:] == 0).all())
    assert bool((G[:, :, :j0, E:].abs().amax((0, 1, 3)) > 0).all())
    check(G, M, qkv, out, H, scale, True)


def test_no_t_by_t_allocation():
    V, N, T, H, E = 4, 2, 256, 2, 32
    M, qkv, out, scale = ar.make_case(3, V, N, T, H, E // H)
    M, qkv, out = M.to(DEV), qkv.to(DEV), out.to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    G = kernels.attention_jac_t(M, qkv, out, H, scale, False)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before - G.numel() * 4
    assert extra < V * N * H * T * T * 4, extra
    check(G, M.cpu(), qkv.cpu(), out.cpu(), H, scale, False)


def test_head_dimension_above_the_kernel_goes_through_the_generic_rule():
    V, N, T, H, d = 3, 2, 5, 1, ar.D_MAX + 1
    M, qkv, out, scale = ar.make_case(9, V, N, T, H, d)
    with pytest.raises(_lib.VivitHipError) as info:
        run(M, qkv, out, H, scale, False)
    assert info.value.status == _lib.VIVIT_E_UNSUPPORTED
    module = ScaledDotProductAttention(H)
    G = _jac_t_mat_prod(module, M.to(DEV), qkv.to(DEV))
    ref, _ = ar.rule(M, qkv, out, H, scale, False)
    torch.testing.assert_close(G.cpu().double(), ref, rtol=1e-4, atol=1e-6)
