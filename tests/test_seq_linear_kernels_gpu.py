"""``kernels.gram_seq_reduce`` (csrc/seq_linear.hip) at the smallest shapes at which it can go wrong, against the fp64 reference under
the derived bound of tests/seq_linear_refs.py (k = T^2 + 3), and what the kernel promises exactly: the bytes of
``gram_hadamard_block`` at T = 1, untouched padding, equal bytes from call to call and for an entry wherever its operands sit."""
import pytest
import torch

import seq_linear_refs as sr
from vivit_amd import kernels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def report(name, got, ref, bound):
    err = (got.cpu().double() - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    print(f"{name}: max error / bound = {ratio:.3g}, max error = {err.max().item():.3g}, max |reference| = {ref.abs().max().item():.3g}")
    ok, msg = sr.within(got.cpu(), ref, bound)
    assert ok, f"{name}: {msg}"


def run_case(seed, Cr, Nr, Cc, Nc, T):
    Gz, Gs, G0 = sr.make_kernel_case(seed, Cr, Nr, Cc, Nc, T)
    Gzd, Gsd = Gz.to(DEV), Gs.to(DEV)
    # beta = 0 over a NaN-filled G: G is not read
    out = torch.full((Cr * Nr, Cc * Nc), float("nan"), device=DEV)
    res = kernels.gram_seq_reduce(Gzd, Gsd, Cr, Nr, Cc, Nc, T, out=out, alpha=1.0, beta=0.0)
    assert res.data_ptr() == out.data_ptr()
    report("beta=0", res, *sr.seq_reduce(Gz, Gs, Cr, Nr, Cc, Nc, T))
    assert torch.equal(kernels.gram_seq_reduce(Gzd, Gsd, Cr, Nr, Cc, Nc, T), res)                  # out=None, and call to call
    # alpha and beta both non-trivial
    res = kernels.gram_seq_reduce(Gzd, Gsd, Cr, Nr, Cc, Nc, T, out=G0.to(DEV), alpha=0.75, beta=-1.5)
    report("alpha,beta", res, *sr.seq_reduce(Gz, Gs, Cr, Nr, Cc, Nc, T, 0.75, -1.5, G0))
    return Gzd, Gsd, G0


@pytest.mark.parametrize("block", sr.KERNEL_BLOCKS, ids=lambda b: "x".join(map(str, b)))
@pytest.mark.parametrize("T", sr.KERNEL_T)
def test_against_reference(T, block):
    run_case(1000 * T + sum(block), *block, T)


@pytest.mark.parametrize("T,Cr,Nr,Cc,Nc", sr.PAST_FIRST)
def test_past_the_first_workgroup_in_rows_and_columns(T, Cr, Nr, Cc, Nc):
    jt = sr.outputs_per_group(T)
    assert Cr * Nr > 2 * sr.ROWS_PER_GROUP and Cc * Nc > 2 * jt and (Cc * Nc) % jt != 0 and jt * T <= sr.SPAN
    run_case(7 * T, Cr, Nr, Cc, Nc, T)


@pytest.mark.parametrize("T,Cr,Nr,Cc,Nc", [(1, 2, 3, 3, 5), (1, 3, 7, 2, 4), (4, 2, 3, 3, 5), (5, 3, 7, 2, 4), (16, 2, 3, 2, 4), (65, 1, 2, 7, 4)])
@pytest.mark.parametrize("pad", [(4, 8, 12), (3, 5, 7), (1, 0, 0), (0, 4, 0)], ids=lambda p: "ld+%d+%d+%d" % p)
def test_leading_dimensions_and_padding(T, Cr, Nr, Cc, Nc, pad):
    """Operands and output as column ranges of wider buffers (multiples of 4 wider: still the float4 body where the sizes allow
    it); the padding of G comes back unchanged, and the result has the bytes of the contiguous call."""
    Gz, Gs, G0 = sr.make_kernel_case(31 * T + Cr, Cr, Nr, Cc, Nc, T)
    rows, cols = Cr * Nr, Cc * Nc
    want = kernels.gram_seq_reduce(Gz.to(DEV), Gs.to(DEV), Cr, Nr, Cc, Nc, T, out=G0.to(DEV), alpha=2.0, beta=0.5)
    wz = torch.full((Nr * T, Nc * T + pad[0]), float("nan"), device=DEV)
    ws = torch.full((rows * T, cols * T + pad[1]), float("nan"), device=DEV)
    wz[:, :Nc * T] = Gz.to(DEV)
    ws[:, :cols * T] = Gs.to(DEV)
    buf, view = sr.with_sentinel_padding(rows, cols, cols + pad[2], DEV)
    view.copy_(G0.to(DEV))
    got = kernels.gram_seq_reduce(wz[:, :Nc * T], ws[:, :cols * T], Cr, Nr, Cc, Nc, T, out=view, alpha=2.0, beta=0.5)
    assert got.data_ptr() == buf.data_ptr() and sr.padding_untouched(buf, cols)
    assert torch.equal(got, want)
    report("padded", got, *sr.seq_reduce(Gz, Gs, Cr, Nr, Cc, Nc, T, 2.0, 0.5, G0))


@pytest.mark.parametrize("which", ["Gz", "Gs", "out", "all"])
@pytest.mark.parametrize("T,Cr,Nr,Cc,Nc", [(1, 2, 3, 3, 8), (4, 2, 3, 3, 5), (16, 2, 3, 2, 4), (65, 1, 2, 7, 4)])
def test_misaligned_operands(T, Cr, Nr, Cc, Nc, which):
    """``data_ptr() % 16 == 4``: the scalar body, and the bytes of the aligned call."""
    Gz, Gs, G0 = sr.make_kernel_case(17 * T + Cc, Cr, Nr, Cc, Nc, T)
    ops = {"Gz": Gz.to(DEV), "Gs": Gs.to(DEV), "out": G0.to(DEV)}
    want = kernels.gram_seq_reduce(ops["Gz"], ops["Gs"], Cr, Nr, Cc, Nc, T, out=G0.to(DEV), alpha=2.0, beta=1.0)
    for name in (ops if which == "all" else [which]):
        ops[name] = sr.misaligned(ops[name])
    got = kernels.gram_seq_reduce(ops["Gz"], ops["Gs"], Cr, Nr, Cc, Nc, T, out=ops["out"], alpha=2.0, beta=1.0)
    assert got.data_ptr() % 16 == (4 if which in ("out", "all") else 0)
    assert torch.equal(got, want)
    report("misaligned", got, *sr.seq_reduce(Gz, Gs, Cr, Nr, Cc, Nc, T, 2.0, 1.0, G0))


@pytest.mark.parametrize("Cr,Nr,Cc,Nc", [(1, 1, 1, 1), (2, 3, 3, 5), (3, 7, 2, 4), (3, 8, 1, 8), (4, 120, 4, 64)])
@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (2.0, 1.0), (0.3, -0.7)])
def test_T1_has_the_bytes_of_gram_hadamard_block(Cr, Nr, Cc, Nc, alpha, beta):
    Gz, Gs, G0 = sr.make_kernel_case(Cr + 10 * Nr + 100 * Cc + 1000 * Nc, Cr, Nr, Cc, Nc, 1)
    Gzd, Gsd = Gz.to(DEV), Gs.to(DEV)
    want = kernels.gram_hadamard_block(Gzd, Gsd, Cr, Nr, Cc, Nc, out=G0.to(DEV), alpha=alpha, beta=beta)
    got = kernels.gram_seq_reduce(Gzd, Gsd, Cr, Nr, Cc, Nc, 1, out=G0.to(DEV), alpha=alpha, beta=beta)
    assert torch.equal(got, want)
    if (Cr * Nr * Cc * Nc) % 4 == 0 and Nc % 4 == 0:    # and on the scalar body
        got = kernels.gram_seq_reduce(sr.misaligned(Gzd), Gsd, Cr, Nr, Cc, Nc, 1, out=G0.to(DEV), alpha=alpha, beta=beta)
        assert torch.equal(got, want)


@pytest.mark.parametrize("T", [2, 5, 16, 65, 130])
def test_an_entry_depends_on_its_operand_blocks_alone(T):
    """The T x T blocks of one sample pair, placed at another block position inside another batch size and class count, give the
    same bytes (the summation order depends on T alone).  The small problem is (Cr, Nr, Cc, Nc) = (1, 2, 1, 2); its blocks are
    planted in a (3, 5, 2, 7) problem, beyond the first workgroup of columns for the larger T."""
    Gz, Gs, G0 = sr.make_kernel_case(5 * T, 1, 2, 1, 2, T)
    small = kernels.gram_seq_reduce(Gz.to(DEV), Gs.to(DEV), 1, 2, 1, 2, T, out=G0.to(DEV), alpha=1.5, beta=0.5).cpu()
    Cr, Nr, Cc, Nc = 3, 5, 2, 7
    BGz, BGs, BG0 = sr.make_kernel_case(5 * T + 1, Cr, Nr, Cc, Nc, T)
    rows_n, cols_m, c, e = (1, 4), (2, 6), 2, 1               # the samples and classes the small problem's rows / columns become
    for i, n in enumerate(rows_n):
        for j, m in enumerate(cols_m):
            BGz[n * T:(n + 1) * T, m * T:(m + 1) * T] = Gz[i * T:(i + 1) * T, j * T:(j + 1) * T]
            r, q = c * Nr + n, e * Nc + m
            BGs[r * T:(r + 1) * T, q * T:(q + 1) * T] = Gs[i * T:(i + 1) * T, j * T:(j + 1) * T]
            BG0[r, q] = G0[i, j]
    big = kernels.gram_seq_reduce(BGz.to(DEV), BGs.to(DEV), Cr, Nr, Cc, Nc, T, out=BG0.to(DEV), alpha=1.5, beta=0.5).cpu()
    for i, n in enumerate(rows_n):
        for j, m in enumerate(cols_m):
            assert big[c * Nr + n, e * Nc + m].item() == small[i, j].item(), (i, j)


def test_launcher_refuses_wrong_shapes():
    Gz, Gs = torch.zeros(6, 10, device=DEV), torch.zeros(12, 30, device=DEV)
    with pytest.raises(ValueError):
        kernels.gram_seq_reduce(Gz, Gs, 2, 3, 3, 5, 3)
    with pytest.raises(ValueError):
        kernels.gram_seq_reduce(Gz, Gs, 2, 3, 3, 5, 2, out=torch.zeros(6, 14, device=DEV))
    with pytest.raises(RuntimeError):
        kernels.gram_seq_reduce(Gz.cpu(), Gs.cpu(), 2, 3, 3, 5, 2)
