"""The five kernels of the Embedding rule (csrc/embedding.hip: ``kernels.embedding_compact``, ``embedding_gram``, ``embedding_vmp``,
``embedding_vtmp``, ``embedding_weight_mjp``) at their edge shapes against the fp64 references under the derived bounds of
tests/embedding_refs.py, and the structure the Gram kernel promises exactly: zeros for samples without a common token, symmetry,
equal bytes from call to call and for a sample pair whatever the batch around it, no tensor with a vocabulary axis."""
import pytest
import torch

import embedding_refs as er
from vivit_amd import kernels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = er.CASES   # the list and what it is a product of: tests/embedding_refs.py


def report(name, got, ref, bound):
    err = (got.cpu().double() - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    print(f"{name}: max error / bound = {ratio:.3g}, max error = {err.max().item():.3g}, max |reference| = {ref.abs().max().item():.3g}")
    ok, msg = er.within(got.cpu(), ref, bound)
    assert ok, f"{name}: {msg}"


def compact(case):
    return kernels.embedding_compact(case.M.to(DEV), case.idx.to(DEV), case.padding_idx)


def check_compact(case, B, ids):
    want = case.ids()
    got = ids.cpu().long()
    assert ids.dtype == torch.int32 and torch.equal(got, want)
    used = got >= 0
    assert bool((used[:, 1:] <= used[:, :-1]).all())                                   # tokens first, then -1
    assert bool((got[:, 1:] > got[:, :-1])[used[:, 1:]].all())                         # strictly increasing
    assert bool((B.cpu()[:, ~used] == 0).all())                                        # rows of -1 slots are exactly zero
    report("compact", B, *case.compact())


def check_gram(case, G, alpha=1.0, beta=0.0, G0=None):
    V, N = case.V, case.N
    ref, bound = case.gram(alpha, beta, G0)
    report("gram", G, ref, bound)
    assert torch.equal(G, G.T)
    if beta == 0.0:
        blocks = G.cpu().view(V, N, V, N)
        disjoint = case.shared_tokens() == 0
        assert bool((blocks.permute(1, 3, 0, 2)[disjoint] == 0).all())                  # no common token: an exactly zero V x V block


def check_all(case, pattern):
    """Every kernel of the rule on one case: compact, gram (symmetry, exact zero blocks), weight_mjp, vmp, vtmp."""
    V, N, D, W = case.V, case.N, case.D, case.W
    B, ids = compact(case)
    check_compact(case, B, ids)
    G = kernels.embedding_gram(B, ids)
    check_gram(case, G)
    if pattern == "allpad":
        assert bool((B == 0).all()) and bool((G == 0).all()) and bool((ids == -1).all())
    # the explicit factor, and the Gram matrix formed from it in fp64: both are within the Gram bound of the truth
    Vt = kernels.embedding_weight_mjp(B, ids, W)
    assert tuple(Vt.shape) == (V, N, W, D)
    report("weight_mjp", Vt, *case.factor())
    flat = Vt.cpu().double().reshape(V * N, W * D)
    ok, msg = er.within(G.cpu(), flat @ flat.T, 2 * case.gram()[1])
    assert ok, f"gram against the explicit factor: {msg}"
    g = er.gen(7)
    mat = torch.randn(2, V, N, generator=g)
    out = kernels.embedding_vmp(B, ids, mat.to(DEV), W)
    ref, bound = case.vmp(mat)
    report("vmp", out, ref, bound)
    ok, msg = er.within(out.cpu(), torch.einsum("fvn,vnwd->fwd", mat.double(), Vt.cpu().double()), 2 * bound)
    assert ok, f"vmp against mat @ factor: {msg}"
    if pattern == "allpad":
        assert bool((out == 0).all())
    mat = torch.randn(2, W, D, generator=g)
    out = kernels.embedding_vtmp(B, ids, mat.to(DEV))
    ref, bound = case.vtmp(mat)
    report("vtmp", out, ref, bound)
    ok, msg = er.within(out.cpu(), torch.einsum("fwd,vnwd->fvn", mat.double(), Vt.cpu().double()), 2 * bound)
    assert ok, f"vtmp against mat @ factor^T: {msg}"


@pytest.mark.parametrize("T,D,V,N,W,pattern,pad", CASES)
def test_edge_shapes(T, D, V, N, W, pattern, pad):
    check_all(er.case_of(T, D, V, N, W, pattern, pad), pattern)


@pytest.mark.parametrize("N,T,S,V,D", er.STAIRCASE_CASES)
def test_token_tables_at_the_edge_of_a_join_pass(N, T, S, V, D):
    """Staircase token patterns (tests/embedding_refs.py): token tables of 256, 257 and 275 entries, tokens shared on both sides of
    the edge between two passes of the join and across sample blocks, under two and three class chunks."""
    case = er.staircase_of(N, T, S, V, D)
    er.check_staircase(case, N, T, S)
    check_all(case, "staircase")


@pytest.mark.parametrize("pad", [False, True], ids=["nopad", "pad"])
def test_token_ids_at_the_top_of_int32(pad):
    """Tokens up to 2^31 - 2: the padding key 2^31 - 1 of the sort and the unsigned order of the id rows (-1 behind every token).
    An output with a vocabulary axis cannot exist here: compact and gram only."""
    case = er.large_id_case(pad)
    B, ids = compact(case)
    check_compact(case, B, ids)
    assert int(ids.max()) == er.I32_MAX - 1 and int((ids >= 0).sum()) == 2 * case.T - (1 if pad else 0)
    G = kernels.embedding_gram(B, ids)
    check_gram(case, G)
    assert bool((G.cpu().view(case.V, 2, case.V, 2)[:, 0, :, 1] != 0).all())      # the samples share two tokens


def test_classes_do_not_depend_on_their_chunk():
    """The Gram matrix of the classes 2 and 7 alone (one class chunk) against their blocks of the matrix of all nine (chunks 0 and
    1): tokens in ascending order and columns in a fixed order whatever wave and accumulator a class pair lands on, equal bytes."""
    V, N, T, D, W = 9, 17, 5, 20, 7
    case = er.make_case(8, V, N, T, D, W, "random")
    G = kernels.embedding_gram(*compact(case))
    check_gram(case, G)
    sel = [2, 7]
    assert sel[0] // er.CLASS_CHUNK != sel[1] // er.CLASS_CHUNK
    two = er.Case(case.M[sel].contiguous(), case.idx, W)
    G2 = kernels.embedding_gram(*compact(two))
    check_gram(two, G2)
    assert torch.equal(G.view(V, N, V, N)[sel][:, :, sel], G2.view(2, N, 2, N))


@pytest.mark.parametrize("D", [4, 20, 128])
def test_compact_form_four_bytes_off_a_16_byte_boundary(D):
    """D % 4 == 0 with a B that is not 16-byte aligned: the scalar load body of the Gram kernel, same arithmetic, same bytes."""
    V, N, T, W = 5, 17, 5, 7
    case = er.make_case(9 + D, V, N, T, D, W, "random")
    B, ids = compact(case)
    Bs = er.misaligned(B)
    assert B.data_ptr() % 16 == 0 and Bs.data_ptr() % 16 == 4 and Bs.is_contiguous() and torch.equal(B, Bs)
    G = kernels.embedding_gram(Bs, ids)
    check_gram(case, G)
    assert torch.equal(G, kernels.embedding_gram(B, ids))
    g = er.gen(7)
    mat = torch.randn(2, V, N, generator=g).to(DEV)
    out = kernels.embedding_vmp(Bs, ids, mat, W)
    report("vmp", out, *case.vmp(mat.cpu()))
    assert torch.equal(out, kernels.embedding_vmp(B, ids, mat, W))
    mat = torch.randn(2, W, D, generator=g).to(DEV)
    out = kernels.embedding_vtmp(Bs, ids, mat)
    report("vtmp", out, *case.vtmp(mat.cpu()))
    assert torch.equal(out, kernels.embedding_vtmp(B, ids, mat))


def test_disjoint_samples_give_exact_zero_blocks():
    """20 samples (two sample blocks) with tokens of their own, except 3 and 18, which share one: every other off-diagonal V x V block
    is exactly zero (checked in check_gram), that one is not."""
    V, N, T, D, W = 3, 20, 5, 20, 100
    case = er.make_case(1, V, N, T, D, W, "distinct")
    idx = case.idx.clone()
    idx[18, 2] = idx[3, 4]
    case = er.Case(case.M, idx, W)
    B, ids = compact(case)
    G = kernels.embedding_gram(B, ids)
    check_gram(case, G)
    shared = case.shared_tokens()
    assert shared[3, 18] == 1 and int((shared > 0).sum()) == N + 2
    assert bool((G.cpu().view(V, N, V, N)[:, 18, :, 3] != 0).all())


def test_bytes_do_not_depend_on_the_call_or_the_batch():
    V, N, T, D, W = 3, 5, 17, 20, 7
    case = er.make_case(2, V, N, T, D, W, "random")
    B, ids = compact(case)
    G1, G2 = kernels.embedding_gram(B, ids), kernels.embedding_gram(B, ids)
    assert torch.equal(G1, G2)
    pair = er.Case(case.M[:, 1:3].contiguous(), case.idx[1:3].contiguous(), W)
    Bp, idsp = compact(pair)
    Gp = kernels.embedding_gram(Bp, idsp)
    assert torch.equal(G1.view(V, N, V, N)[:, 1:3][:, :, :, 1:3], Gp.view(V, 2, V, 2))


def test_bytes_of_a_pair_across_sample_blocks():
    """Samples 2 and 30 of a batch of 33 (two sample blocks apart) against the batch that holds only those two."""
    V, N, T, D, W = 3, 33, 5, 67, 7
    case = er.make_case(3, V, N, T, D, W, "random")
    B, ids = compact(case)
    G = kernels.embedding_gram(B, ids).view(V, N, V, N)
    sel = [2, 30]
    pair = er.Case(case.M[:, sel].contiguous(), case.idx[sel].contiguous(), W)
    Gp = kernels.embedding_gram(*compact(pair))
    assert torch.equal(G[:, sel][:, :, :, sel], Gp.view(V, 2, V, 2))


@pytest.mark.parametrize("alpha,beta", [(1.0, 1.0), (0.5, -2.0)])
def test_out_and_beta_accumulate(alpha, beta):
    for V in (3, 5):                                                 # one class chunk; two: mirror writes across chunks
        N, T, D, W = 17, 5, 20, 7
        case = er.make_case(4, V, N, T, D, W, "random", 0)
        B, ids = compact(case)
        prior = kernels.embedding_gram(*compact(er.make_case(5, V, N, T, D, W, "random")))
        G0 = prior.clone()
        out = kernels.embedding_gram(B, ids, out=prior, alpha=alpha, beta=beta)
        assert out.data_ptr() == prior.data_ptr()
        check_gram(case, out, alpha, beta, G0.cpu())


def test_no_materialisation():
    """Vocabulary 50 000: compact form and Gram matrix stay below the size of the explicit factor (307 MB) by orders."""
    V, N, T, D, W = 3, 8, 8, 64, 50000
    case = er.make_case(6, V, N, T, D, W, "random")
    M, idx = case.M.to(DEV), case.idx.to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    B, ids = kernels.embedding_compact(M, idx)
    G = kernels.embedding_gram(B, ids)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f"peak extra memory {extra} bytes, explicit factor {V * N * W * D * 4} bytes")
    assert extra < V * N * W * D * 4, extra
    assert extra < 1 << 20, extra                                    # O(V N T D + n^2): 48 KiB of B, 2 KiB of G, the sort's buffers
    check_compact(case, B, ids)
    check_gram(case, G)
