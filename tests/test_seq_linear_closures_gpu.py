"""``_linear_seq_weight_closures`` (vivit_amd/backend/extensions.py) against the explicit factor in fp64 under the closure bounds of
tests/seq_linear_refs.py: both routes of ``gram_mat`` (the route is forced through ``SEQ_LINEAR_KAPPA``, the slabs and chunks through
``SEQ_LINEAR_WORKSPACE_BYTES``, both read at call time), the two products, ``factor()``, and the memory the Gram build takes."""
import pytest
import torch
from torch import nn

import seq_linear_refs as sr
from vivit_amd import kernels
from vivit_amd.backend import ViViTGGNExact
from vivit_amd.backend import extensions as ext

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MIB = 1 << 20

# id: (C, N, A, O, I, route, budget or None, slabs / chunks the plan must have).  Budget, route A: the bytes a slab of Gs may take
# (half the workspace constant); route B: the output features of a chunk (the constant is that chunk plus its SYRK's scratch buffer)
CASES = {
    "A-one-slab": (3, 5, (4,), 6, 7, "A", None, [(0, 15)]),
    "A-sample-slabs": (2, 9, (3,), 5, 4, "A", 1440, [(0, 6), (6, 9), (9, 12), (12, 14), (14, 16), (16, 18)]),
    "A-class-slabs": (4, 3, (2,), 5, 4, "A", 4 * 4 * 60, [(0, 6), (6, 9), (9, 12)]),
    "B-chunks": (2, 4, (6,), 11, 5, "B", 4, [(0, 4), (4, 8), (8, 11)]),
    "B-one-chunk": (3, 5, (4,), 6, 7, "B", None, [(0, 6)]),
    "A-extra-dims": (2, 3, (2, 3), 5, 4, "A", None, [(0, 6)]),
    "B-extra-dims": (2, 3, (2, 3), 5, 4, "B", 2, [(0, 2), (2, 4), (4, 5)]),
    "A-T17": (2, 3, (17,), 3, 9, "A", 4 * 17 * 17 * 14, [(0, 3), (3, 5), (5, 6)]),
}


def workspace_for(route, budget, C, N, I):
    if budget is None:
        return None
    if route == "A":
        return 2 * budget
    return 4 * C * N * budget * I + kernels.gram_syrk_workspace_bytes(C * N, budget * I)


def report(name, got, ref, bound):
    err = (got.cpu().double() - ref).abs()
    print(f"{name}: max error / bound = {(err / bound.clamp_min(1e-300)).max().item():.3g}, max error = {err.max().item():.3g}, "
          f"max |reference| = {ref.abs().max().item():.3g}")
    ok, msg = sr.within(got.cpu(), ref, bound)
    assert ok, f"{name}: {msg}"


def force(monkeypatch, route, W):
    monkeypatch.setattr(ext, "SEQ_LINEAR_KAPPA", 0.0 if route == "A" else 1e30)
    if W is not None:
        monkeypatch.setattr(ext, "SEQ_LINEAR_WORKSPACE_BYTES", W)


def spy(monkeypatch, name):
    calls = []
    real = getattr(kernels, name)

    def wrapped(*a, **k):
        calls.append(name)
        return real(*a, **k)

    monkeypatch.setattr(kernels, name, wrapped)
    return calls


def check_slab_calls(monkeypatch, cl, slabs, C, N, T):
    """What route A asks of ``kernels.gram_seq_reduce``: from the block sizes and the place of ``out`` in G of every call, the
    calls of a slab cover its rows against exactly the columns 0 .. cols - 1 = 0 .. r1 - 1, each entry once, so every entry on
    or below the diagonal is computed once over all slabs and none beyond a slab's own last row."""
    n = C * N
    G = torch.zeros(C, N, C, N, device=DEV)
    count = torch.zeros(n, n, dtype=torch.int64)
    real = kernels.gram_seq_reduce

    def counting(Gz, Gs, Cr, Nr, Cc, Nc, Tk, out=None, alpha=1.0, beta=0.0):
        assert Tk == T and tuple(out.shape) == (Cr * Nr, Cc * Nc) and tuple(Gs.shape) == (Cr * Nr * T, Cc * Nc * T)
        off = (out.data_ptr() - G.data_ptr()) // 4
        assert out.stride(0) == n and 0 <= off < n * n
        r, c = divmod(off, n)
        count[r:r + Cr * Nr, c:c + Cc * Nc] += 1
        return real(Gz, Gs, Cr, Nr, Cc, Nc, Tk, out=out, alpha=alpha, beta=beta)

    with monkeypatch.context() as m:
        m.setattr(kernels, "gram_seq_reduce", counting)
        cl["gram_mat"](out=G, beta=0.0)
    want = torch.zeros(n, n, dtype=torch.int64)
    for r0, r1, cols in slabs:
        assert cols == r1
        want[r0:r1, :cols] = 1
    assert torch.equal(count, want), "the calls of a slab do not cover exactly its rows against the columns up to its last row"
    low = torch.tril(torch.ones(n, n, dtype=torch.int64))
    assert torch.equal(count * low, low)


def check_closures(monkeypatch, p, s_dev, z_dev, route, W, want_plan):
    C, N, T, O, I = p.C, p.N, p.T, p.O, p.I
    n = C * N
    force(monkeypatch, route, W)
    plan = ext._seq_linear_plan(C, N, T, O, I)
    assert plan["route"] == route
    units = plan["slabs"] if route == "A" else plan["chunks"]
    if want_plan is not None:
        assert (sr.slab_rows(units) if route == "A" else units) == want_plan
    reduces, convs = spy(monkeypatch, "gram_seq_reduce"), spy(monkeypatch, "conv2d_weight_mjp")
    cl = ext._linear_seq_weight_closures(s_dev, z_dev)
    assert set(cl) == {"V_mat_prod", "V_t_mat_prod", "gram_mat", "factor", "shape_cn", "dp_add"} and cl["shape_cn"] == (C, N)
    bound = p.bound_A() if route == "A" else p.bound_B(len(units), max(o1 - o0 for o0, o1 in units))

    G = cl["gram_mat"]()
    assert tuple(G.shape) == (C, N, C, N) and G.is_contiguous()
    G2d = G.view(n, n)
    assert torch.equal(G2d, G2d.T), "gram_mat is not exactly symmetric"
    report(f"gram_mat route {route}", G2d, p.G, bound)
    if route == "A":
        assert len(reduces) >= len(units) and not convs
        check_slab_calls(monkeypatch, cl, units, C, N, T)
    else:
        assert len(convs) == len(units) and not reduces
    assert torch.equal(cl["gram_mat"]().view(n, n), G2d)                       # call to call

    # out / beta = 1 onto a symmetric prior; beta = 0 over NaN
    g = sr.gen(11)
    prior = sr.generic(g, n, n)
    prior = (prior + prior.T).contiguous() * float(p.G.abs().max()) ** 0.5
    out = prior.to(DEV).view(C, N, C, N).clone()
    res = cl["gram_mat"](out=out, beta=1.0)
    assert res.data_ptr() == out.data_ptr() and torch.equal(out.view(n, n), out.view(n, n).T)
    report("gram_mat beta=1", out.view(n, n), p.G + prior.double(), bound + p.prior_bound(prior, 1.0))
    out = torch.full((C, N, C, N), float("nan"), device=DEV)
    assert torch.equal(cl["gram_mat"](out=out, beta=0.0).view(n, n), G2d)

    mat = torch.randn(3, C, N, generator=g)
    report("V_mat_prod", cl["V_mat_prod"](mat.to(DEV)), *p.vmp(mat))
    mat = torch.randn(3, O, I, generator=g)
    report("V_t_mat_prod", cl["V_t_mat_prod"](mat.to(DEV)), *p.vtmp(mat))

    monkeypatch.undo()
    V = cl["factor"]()
    assert tuple(V.shape) == (C, N, O, I)
    assert torch.equal(V, ext._param_factor(nn.Linear(I, O), "weight", s_dev, z_dev))
    report("factor", V, p.V, sr.gamma(T + 1) * torch.einsum("cnto,nti->cnoi", p.s4.abs(), p.z3.abs()) + sr.tau(T) * p.V.abs().max())


@pytest.mark.parametrize("case", CASES)
def test_closures(case, monkeypatch):
    C, N, A, O, I, route, W, want = CASES[case]
    p = sr.make_problem(sum(map(ord, case)), C, N, A, O, I)
    check_closures(monkeypatch, p, p.s.to(DEV), p.z.to(DEV), route, workspace_for(route, W, C, N, I), want)


@pytest.mark.parametrize("route", ["A", "B"])
def test_non_contiguous_operands(route, monkeypatch):
    """``M`` as a transposed view and as every other row of a wider tensor, ``x`` as a column range."""
    C, N, T, O, I = 2, 3, 4, 5, 6
    p = sr.make_problem(41, C, N, (T,), O, I)
    s_dev = p.s.to(DEV).permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    wide = torch.zeros(N, T, 2 * I + 1, device=DEV)
    wide[..., 1:2 * I:2] = p.z.to(DEV)
    z_dev = wide[..., 1:2 * I:2]
    assert not s_dev.is_contiguous() and not z_dev.is_contiguous()
    check_closures(monkeypatch, p, s_dev, z_dev, route, None, None)


def test_store_takes_the_closures_above_the_threshold_only(monkeypatch):
    C, N, T, O, I = 2, 3, 4, 5, 6
    p = sr.make_problem(43, C, N, (T,), O, I)
    module = nn.Linear(I, O).to(DEV)
    made = []
    real = ext._linear_seq_weight_closures
    monkeypatch.setattr(ext, "_linear_seq_weight_closures", lambda s, z: made.append(1) or real(s, z))
    e = ViViTGGNExact()
    e._store(module, "weight", module.weight, p.s.to(DEV), p.z.to(DEV))
    assert not made                                                             # 4 C N O I = 720 bytes, far below 64 MiB
    explicit = module.weight.vivit_ggn_exact["gram_mat"]()
    monkeypatch.setattr(ext, "SEQ_LINEAR_EXPLICIT_MAX_BYTES", 4 * C * N * O * I)
    e._store(module, "weight", module.weight, p.s.to(DEV), p.z.to(DEV))
    assert not made                                                             # "would exceed": equal is not above
    monkeypatch.setattr(ext, "SEQ_LINEAR_EXPLICIT_MAX_BYTES", 4 * C * N * O * I - 1)
    e._store(module, "weight", module.weight, p.s.to(DEV), p.z.to(DEV))
    assert made == [1]
    report("against today's path", module.weight.vivit_ggn_exact["gram_mat"]().view(C * N, C * N), explicit.cpu().double().view(C * N, C * N),
           2 * torch.minimum(p.bound_A(), p.bound_B(1, O)))
    e._store(module, "bias", module.bias, p.s.to(DEV), p.z.to(DEV))             # a bias, a host tensor, fp64: today's path
    e._store(module, "weight", module.weight, p.s.double().to(DEV), p.z.double().to(DEV))
    cpu = nn.Linear(I, O)
    e._store(cpu, "weight", cpu.weight, p.s, p.z)
    assert made == [1]


# ---- memory ---------------------------------------------------------------------------------------------------------------------
MEM = (4, 16, 4, 256, 256)      # the explicit factor is 16 MiB, route A's Gs 256 KiB


def peak_of_gram(monkeypatch, route, W):
    """(peak bytes above the operands during gram_mat(), conv2d_weight_mjp calls, gram_seq_reduce calls), through ``_store``."""
    C, N, T, O, I = MEM
    g = sr.gen(3)
    s, z = torch.randn(C, N, T, O, generator=g).to(DEV), torch.randn(N, T, I, generator=g).to(DEV)
    module = nn.Linear(I, O).to(DEV)
    monkeypatch.setattr(ext, "SEQ_LINEAR_EXPLICIT_MAX_BYTES", 0, raising=False)
    monkeypatch.setattr(ext, "SEQ_LINEAR_KAPPA", 1.0 if route == "A" else 1e30, raising=False)
    if W is not None:
        monkeypatch.setattr(ext, "SEQ_LINEAR_WORKSPACE_BYTES", W, raising=False)
    convs, reduces = spy(monkeypatch, "conv2d_weight_mjp"), []
    if hasattr(kernels, "gram_seq_reduce"):
        reduces = spy(monkeypatch, "gram_seq_reduce")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ViViTGGNExact()._store(module, "weight", module.weight, s, z)
    G = module.weight.vivit_ggn_exact["gram_mat"]()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"route {route}: peak {peak / MIB:.3f} MiB above the operands, {len(convs)} conv2d_weight_mjp, {len(reduces)} gram_seq_reduce")
    ref = torch.einsum("cnto,nti->cnoi", s.double(), z.double()).reshape(C * N, O * I)
    assert ((G.view(C * N, C * N).double() - ref @ ref.T).abs().max() / (ref @ ref.T).abs().max()).item() < 1e-4
    return peak, convs, reduces


def test_route_A_memory_is_a_fraction_of_the_factor(monkeypatch):
    """With kappa = 1 the planner itself takes route A here (16 times fewer multiply-adds)."""
    peak, convs, reduces = peak_of_gram(monkeypatch, "A", None)
    assert not convs, "the explicit factor was built"
    assert len(reduces) == 1
    assert peak < 4 * MIB                                                       # a quarter of the factor: a condition, not a measurement


def test_route_B_memory_is_the_workspace(monkeypatch):
    peak, convs, reduces = peak_of_gram(monkeypatch, "B", 2 * MIB)
    C, N, T, O, I = MEM
    chunks = ext._seq_linear_plan(C, N, T, O, I, workspace_bytes=2 * MIB, kappa=1e30)["chunks"]
    assert len(convs) == len(chunks) >= 8 and not reduces                       # a chunk and the scratch of its SYRK within 2 MiB
    assert peak < 2 * MIB + 1 * MIB


# ---- the pieces of route A's products and the scratch buffer of the launchers ----------------------------------------------------
@pytest.mark.parametrize("m,nb,k,cap", [(37, 53, 19, 200), (64, 64, 8, 100), (5, 300, 7, 64), (130, 3, 11, 50), (33, 47, 5, 10 ** 9)])
def test_gemm_nt_within_cuts_into_ragged_pieces(m, nb, k, cap, monkeypatch):
    """With the piece floor lowered and a scratch query that charges m x n bytes, the product is cut until a piece is within
    ``cap`` (ragged last pieces, ``out`` slices with the full leading dimension); the result is the product, and where nothing is
    cut it has the bytes of one ``gemm_nt``."""
    g = sr.gen(m + nb + k)
    A, B = sr.generic(g, m, k), sr.generic(g, nb, k)
    pieces = []
    real = kernels.gemm_nt
    monkeypatch.setattr(ext, "GEMM_PIECE_MIN_ROWS", 2)
    monkeypatch.setattr(kernels, "gemm_workspace_bytes", lambda mm, nn_, kk: mm * nn_)
    monkeypatch.setattr(kernels, "gemm_nt", lambda a, b, out=None, **kw: pieces.append((a.shape[0], b.shape[0])) or real(a, b, out=out, **kw))
    got = ext._gemm_nt_within(A.to(DEV), B.to(DEV), cap)
    ref = A.double() @ B.double().T
    report("pieces", got, ref, torch.full_like(ref, sr.tau(k) * float(ref.abs().max())))
    assert sum(a * b for a, b in pieces) == m * nb
    if m * nb <= cap:
        assert pieces == [(m, nb)] and torch.equal(got, real(A.to(DEV), B.to(DEV)))
    else:
        assert len(pieces) > 1 and all(a * b <= cap or max(a, b) <= 2 for a, b in pieces)
        assert len({p for p in pieces}) > 1 or (m % pieces[0][0] == 0 and nb % pieces[0][1] == 0)


def test_gram_within_falls_back_to_pieces(monkeypatch):
    g = sr.gen(9)
    A = sr.generic(g, 45, 13)
    ref = A.double() @ A.double().T
    bound = torch.full_like(ref, sr.tau(13) * float(ref.abs().max()))
    syrks, gemms = spy(monkeypatch, "gram_syrk"), spy(monkeypatch, "gemm_nt")
    report("syrk", ext._gram_within(A.to(DEV), 1 << 30), ref, bound)
    assert len(syrks) == 1 and not gemms
    monkeypatch.setattr(ext, "GEMM_PIECE_MIN_ROWS", 2)
    monkeypatch.setattr(kernels, "gram_syrk_workspace_bytes", lambda n, p: 1 << 40)
    monkeypatch.setattr(kernels, "gemm_workspace_bytes", lambda mm, nn_, kk: mm * nn_)
    report("pieces", ext._gram_within(A.to(DEV), 300), ref, bound)
    assert len(syrks) == 1 and len(gemms) > 1


def test_route_A_with_cut_products(monkeypatch):
    """Route A end to end with Gz and every slab of Gs built in pieces."""
    monkeypatch.setattr(ext, "GEMM_PIECE_MIN_ROWS", 2)
    monkeypatch.setattr(kernels, "gram_syrk_workspace_bytes", lambda n, p: 1 << 40)
    monkeypatch.setattr(kernels, "gemm_workspace_bytes", lambda mm, nn_, kk: 64 * mm * nn_)
    C, N, A, O, I, route, W, want = CASES["A-class-slabs"]
    p = sr.make_problem(77, C, N, A, O, I)
    force(monkeypatch, route, workspace_for(route, W, C, N, I))
    gemms = spy(monkeypatch, "gemm_nt")
    cl = ext._linear_seq_weight_closures(p.s.to(DEV), p.z.to(DEV))
    G = cl["gram_mat"]().view(C * N, C * N)
    assert len(gemms) > 1 + len(want) and torch.equal(G, G.T)
    report("gram_mat, cut products", G, p.G, p.bound_A())


def test_workspace_is_released_before_it_grows():
    """``kernels._workspace``: a larger request replaces the cached buffer without the two coexisting, a smaller one reuses it, and
    a product computed after the growth is the product."""
    like = torch.zeros(1, device=DEV)
    kernels._WORKSPACES.clear()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    small, big = 6 * MIB, 20 * MIB
    p1, n1 = kernels._workspace(small, like)
    assert n1 == kernels._workspace_alloc_bytes(small) and n1 <= torch.cuda.memory_allocated() - base < n1 + 2 * MIB   # (the allocator's blocks: 2 MiB granules at most)
    assert kernels._workspace(small - 1, like) == (p1, n1) and kernels._workspace(0, like) == (None, 0)
    torch.cuda.reset_peak_memory_stats()
    p2, n2 = kernels._workspace(big, like)
    assert n2 == kernels._workspace_alloc_bytes(big) >= big
    assert n2 <= torch.cuda.memory_allocated() - base < n2 + 2 * MIB
    assert torch.cuda.max_memory_allocated() - base < n1 + n2, "the old and the new scratch buffer coexisted"
    assert kernels._workspace(small, like) == (p2, n2) and len(kernels._WORKSPACES) == 1
    g = sr.gen(1)
    A = sr.generic(g, 300, 70)
    ref = A.double() @ A.double().T
    report("syrk after growth", kernels.gram_syrk(A.to(DEV)), ref, torch.full_like(ref, sr.tau(70) * float(ref.abs().max())))
    kernels._WORKSPACES.clear()

