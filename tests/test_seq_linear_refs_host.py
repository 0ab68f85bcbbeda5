"""tests/seq_linear_refs.py checked on the host (no GPU): the references against the explicit fp64 factor, the bounds against a
plain fp32 evaluation and against deliberately wrong formulas, the tiling constants against the kernel source, and the planner
``_seq_linear_plan`` of vivit_amd/backend/extensions.py directly."""
import math
import os
import re

import pytest
import torch

import seq_linear_refs as sr
from vivit_amd import kernels
from vivit_amd.backend import extensions as ext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = sr.F64


@pytest.mark.parametrize("C,N,T,O,I", sr.IDENTITY_SHAPES)
def test_expanded_formula_is_the_gram_matrix_of_the_explicit_factor(C, N, T, O, I):
    p = sr.make_problem(C + 10 * N + 100 * T, C, N, (T,), O, I)
    G, mag = p.gram_expanded()
    assert p.V.shape == (C, N, O, I) and p.T == T
    assert (G - p.G).abs().max().item() <= 1e-12 * max(p.G.abs().max().item(), 1e-300)
    assert bool((mag >= G.abs() * (1 - 1e-12)).all())
    explicit = torch.einsum("cnoi,emoi->cnem", p.V, p.V).reshape(C * N, C * N)
    assert (explicit - p.G).abs().max().item() <= 1e-12 * p.G.abs().max().item()


def test_extra_dimensions_flatten_into_T():
    p = sr.make_problem(3, 2, 3, (2, 3), 4, 5)
    assert p.T == 6 and p.V.shape == (2, 3, 4, 5)
    want = torch.einsum("cnabo,nabi->cnoi", p.s.to(F64), p.z.to(F64))
    assert torch.equal(want, p.V) or (want - p.V).abs().max().item() < 1e-12 * p.V.abs().max().item()


KERNEL_HOST = [(T, b) for T in (1, 2, 5, 17, 65) for b in sr.KERNEL_BLOCKS]


def wrong_variants(Gz, Gs, Cr, Nr, Cc, Nc, T):
    """Three wrong evaluations, in fp64: t / u swapped on Gs only; rows of Gs read sample-major; the last u dropped."""
    z = Gz.to(F64).reshape(1, Nr, T, 1, Nc, T)
    s = Gs.to(F64).reshape(Cr, Nr, T, Cc, Nc, T)
    swapped = (z * s.transpose(2, 5)).sum((2, 5)).reshape(Cr * Nr, Cc * Nc)
    sample_major = (z * Gs.to(F64).reshape(Nr, Cr, T, Cc, Nc, T).transpose(0, 1)).sum((2, 5)).reshape(Cr * Nr, Cc * Nc)
    dropped = (z[..., :T - 1] * s[..., :T - 1]).sum((2, 5)).reshape(Cr * Nr, Cc * Nc)
    return {"swapped": swapped, "sample_major": sample_major, "dropped": dropped}


@pytest.mark.parametrize("T,block", KERNEL_HOST, ids=lambda v: str(v).replace(" ", ""))
def test_kernel_bound_holds_for_fp32_and_not_for_wrong_formulas(T, block):
    Cr, Nr, Cc, Nc = block
    Gz, Gs, G0 = sr.make_kernel_case(1000 * T + sum(block), Cr, Nr, Cc, Nc, T)
    for alpha, beta in ((1.0, 0.0), (0.75, -1.5)):
        ref, bound = sr.seq_reduce(Gz, Gs, Cr, Nr, Cc, Nc, T, alpha, beta, G0)
        got = sr.seq_reduce_fp32(Gz, Gs, Cr, Nr, Cc, Nc, T, alpha, beta, G0)
        ok, msg = sr.within(got, ref, bound)
        assert ok, msg
        worst = ((got.to(F64) - ref).abs() / bound.clamp_min(1e-300)).max().item()
        print(f"T={T} {block}: plain fp32 uses {worst:.2f} of the bound")
    ref, bound = sr.seq_reduce(Gz, Gs, Cr, Nr, Cc, Nc, T)
    for name, wrong in wrong_variants(Gz, Gs, Cr, Nr, Cc, Nc, T).items():
        if (name == "swapped" and T == 1) or (name == "sample_major" and (Cr == 1 or Nr == 1)):
            continue                            # the variant is the formula itself there
        assert not sr.within(wrong, ref, bound)[0], f"{name} passes the bound at T={T}, {block}"


@pytest.mark.parametrize("T,block", [(T, b) for T in sr.KERNEL_T for b in sr.KERNEL_BLOCKS], ids=lambda v: str(v).replace(" ", ""))
def test_kernel_reference_against_a_loop(T, block):
    """The vectorised reference restates the formula of include/vivit_hip.h; spot-check it entry by entry."""
    Cr, Nr, Cc, Nc = block
    Gz, Gs, _ = sr.make_kernel_case(1000 * T + sum(block), Cr, Nr, Cc, Nc, T)
    ref, _ = sr.seq_reduce(Gz, Gs, Cr, Nr, Cc, Nc, T)
    for (c, n, e, m) in {(0, 0, 0, 0), (Cr - 1, Nr - 1, Cc - 1, Nc - 1), (Cr - 1, 0, 0, Nc - 1)}:
        r, j = c * Nr + n, e * Nc + m
        want = (Gz.to(F64)[n * T:(n + 1) * T, m * T:(m + 1) * T] * Gs.to(F64)[r * T:(r + 1) * T, j * T:(j + 1) * T]).sum()
        assert abs(ref[r, j].item() - want.item()) <= 1e-12 * max(abs(want.item()), 1e-300)


def test_tiling_constants_are_those_of_the_kernel_source():
    src = open(os.path.join(ROOT, "vivit_amd", "csrc", "seq_linear.hip")).read()
    assert int(re.search(r"constexpr int SR_BLOCK = (\d+);", src).group(1)) == sr.BLOCK
    assert int(re.search(r"constexpr int SR_SPAN = (\d+);", src).group(1)) == sr.SPAN
    assert "SR_T_MAX = SR_SPAN" in src and sr.T_MAX == sr.SPAN
    assert "dim3 grid((unsigned)rows, (unsigned)spans)" in src and sr.ROWS_PER_GROUP == 1
    for T in (1, 2, 3, 4, 5, 6, 16, 17, 63, 64, 65, 130, 197, 256, 257, 341, 342, 512, 513, 1024):
        jt = sr.outputs_per_group(T)
        assert 1 <= jt and jt * T <= sr.SPAN and (jt + 1) * T > sr.SPAN - 3 * T
        assert (jt * T) % 4 == 0 or jt < 4 // math.gcd(T, 4)
    assert [sr.outputs_per_group(T) for T in (2, 5, 16, 65, 130, 197, 600, 1024)] == [512, 204, 64, 12, 6, 4, 1, 1]
    for T, Cr, Nr, Cc, Nc in sr.PAST_FIRST:
        jt = sr.outputs_per_group(T)
        assert Cr * Nr > 2 and Cc * Nc > 2 * jt and (Cc * Nc) % jt != 0


# ---- the closures' bounds -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,N,T,O,I", sr.IDENTITY_SHAPES)
def test_closure_bounds_hold_for_fp32_and_not_for_wrong_wiring(C, N, T, O, I):
    p = sr.make_problem(7 + C + 10 * N + 100 * T, C, N, (T,), O, I)
    s2, z2 = p.s.reshape(C * N * T, O), p.z.reshape(N * T, I)
    Gs32, Gz32 = s2 @ s2.T, z2 @ z2.T
    got = sr.seq_reduce_fp32(Gz32, Gs32, C, N, C, N, T)
    ok, msg = sr.within(got, p.G, p.bound_A())
    assert ok, msg
    V32 = torch.einsum("cnto,nti->cnoi", p.s.reshape(C, N, T, O), p.z.reshape(N, T, I)).reshape(C * N, O * I)
    ok, msg = sr.within(V32 @ V32.T, p.G, p.bound_B(1, O))
    assert ok, msg
    g = sr.gen(5)
    mat = torch.randn(2, C, N, generator=g)
    ref, bound = p.vmp(mat)
    ok, msg = sr.within(torch.einsum("fcn,cnoi->foi", mat, V32.view(C, N, O, I)), ref, bound)
    assert ok, msg
    if T > 1:   # mat not repeated over t: only t = 0 contributes
        wrong = torch.einsum("fcn,cno,ni->foi", mat.to(F64), p.s4[:, :, 0], p.z3[:, 0])
        assert not sr.within(wrong, ref, bound)[0]
    mat = torch.randn(2, O, I, generator=g)
    ref, bound = p.vtmp(mat)
    ok, msg = sr.within(torch.einsum("foi,cnoi->fcn", mat, V32.view(C, N, O, I)), ref, bound)
    assert ok, msg
    if C > 1 and N > 1:
        wrong = torch.einsum("foi,cnoi->fcn", mat.to(F64), p.V).transpose(1, 2).reshape(2, C, N)
        assert not sr.within(wrong, ref, bound)[0]
    for name, wrong in wrong_variants(p.Gz, p.Gs, C, N, C, N, T).items():   # loose as it is, the Gram bound still sees wrong wiring
        if (name == "swapped" and T == 1) or (name == "sample_major" and (C == 1 or N == 1)):
            continue
        if name == "dropped" and T > 8:         # 1 / T of the terms: below this bound's T^2 tau max|Gs| max|Gz|; the kernel bound sees it
            continue
        assert not sr.within(wrong, p.G, p.bound_A())[0], name


# ---- the planner ----------------------------------------------------------------------------------------------------------------
MIB = 1 << 20


def test_constants():
    assert ext.SEQ_LINEAR_WORKSPACE_BYTES == 256 * MIB and ext.SEQ_LINEAR_EXPLICIT_MAX_BYTES == 64 * MIB and ext.SEQ_LINEAR_KAPPA > 0


@pytest.mark.parametrize("T,O,I", [(T, O, I) for T in (4, 16, 64, 197) for (O, I) in ((3072, 768), (768, 3072))])
def test_route_follows_the_multiply_add_counts(T, O, I):
    C, N = 10, 64
    plan = ext._seq_linear_plan(C, N, T, O, I, kappa=1.0)
    n = C * N
    macs_A = (n * T) ** 2 / 2 * O + (N * T) ** 2 / 2 * I
    macs_B = n ** 2 / 2 * O * I + n * T * O * I
    assert plan["macs_A"] == macs_A and plan["macs_B"] == macs_B
    fits = 4 * T * n * T <= ext.SEQ_LINEAR_WORKSPACE_BYTES // 2              # slabs take half the workspace, the GEMMs' scratch the other
    assert plan["route"] == ("A" if fits and macs_A <= macs_B else "B")
    assert bool(plan["slabs"]) == (plan["route"] == "A") and bool(plan["chunks"]) == (plan["route"] == "B")
    if plan["route"] == "A":
        count = sr.check_slabs(plan["slabs"], C, N, T, ext.SEQ_LINEAR_WORKSPACE_BYTES // 2)
        assert bool((torch.tril(count) == torch.tril(torch.ones_like(count))).all())
    else:
        sr.check_chunks(plan["chunks"], C, N, O, I, ext.SEQ_LINEAR_WORKSPACE_BYTES, kernels.gram_syrk_workspace_bytes)


def test_headline_shapes():
    assert ext._seq_linear_plan(10, 64, 16, 3072, 768, kappa=1.0)["route"] == "A"       # 3.0 x fewer multiply-adds
    p = ext._seq_linear_plan(10, 64, 4, 3072, 768, kappa=1.0)
    assert p["route"] == "A" and p["slabs"] == [(0, 640, 640)] and 47 < p["macs_B"] / p["macs_A"] < 49
    assert ext._seq_linear_plan(10, 64, 197, 3072, 768, kappa=1.0)["route"] == "B"
    p = ext._seq_linear_plan(10, 64, 16, 3072, 768, kappa=1.0)
    assert 3.0 < p["macs_B"] / p["macs_A"] < 3.3 and len(p["slabs"]) == 3                # Gs is 400 MiB, a slab 128 MiB at most


def test_kappa_moves_the_crossover_and_is_read_at_call_time(monkeypatch):
    assert ext._seq_linear_plan(3, 5, 4, 6, 7, kappa=1.0)["route"] == "B"
    assert ext._seq_linear_plan(3, 5, 4, 6, 7, kappa=0.0)["route"] == "A"
    assert ext._seq_linear_plan(10, 64, 4, 3072, 768, kappa=100.0)["route"] == "B"
    monkeypatch.setattr(ext, "SEQ_LINEAR_KAPPA", 0.0)
    assert ext._seq_linear_plan(3, 5, 4, 6, 7)["route"] == "A"
    monkeypatch.setattr(ext, "SEQ_LINEAR_WORKSPACE_BYTES", 2 * 4 * 4 * 15 * 4 - 1)      # one row of blocks no longer fits its half
    assert ext._seq_linear_plan(3, 5, 4, 6, 7)["route"] == "B"


@pytest.mark.parametrize("C,N,T,W", [(2, 9, 3, 1440), (2, 9, 3, 4 * 3 * 18 * 3), (4, 3, 2, 4 * 4 * 6 * 7), (4, 3, 2, 4 * 4 * 80), (4, 3, 2, 4 * 4 * 60), (10, 64, 16, 256 * MIB),
                                     (10, 64, 16, 64 * MIB), (3, 5, 4, 1 << 30), (5, 7, 3, 4 * 9 * 35 * 8), (1, 13, 2, 4 * 4 * 40)])
def test_slabs(C, N, T, W):
    """``W``: the bytes a slab may take, half the workspace."""
    plan = ext._seq_linear_plan(C, N, T, 5, 4, workspace_bytes=2 * W, kappa=0.0)
    assert plan["route"] == "A"
    slabs = plan["slabs"]
    count = sr.check_slabs(slabs, C, N, T, W)
    n = C * N
    low = torch.tril(torch.ones(n, n, dtype=torch.int64))
    assert bool((count * low == low).all()), "every lower entry exactly once"
    for r0, r1, cols in slabs:
        assert cols == r1 and int(count[r0:r1, r1:].sum()) == 0, "a slab stops at its own last row"
    if 4 * n * T * n * T <= W:
        assert slabs == [(0, n, n)]
    else:
        assert len(slabs) > 1
        # greedy: a slab could not have taken the next unit (a class after whole classes, a sample within a class)
        for r0, r1, _ in slabs[:-1]:
            if r0 % N == 0 and r1 % N == 0:
                assert 4 * (r1 + N - r0) * T * (r1 + N) * T > W
            elif r1 % N != 0:
                assert 4 * (r1 + 1 - r0) * T * (r1 + 1) * T > W


def test_a_slab_past_its_own_last_row_is_seen():
    """``check_slabs`` counts from the plan's column ends: slabs that run on to the last column compute upper entries, and a slab
    that stops short of its diagonal leaves lower entries out."""
    C, N, T = 4, 3, 2
    slabs = ext._seq_linear_plan(C, N, T, 5, 4, workspace_bytes=2 * 4 * 4 * 60, kappa=0.0)["slabs"]
    n = C * N
    wide = sr.check_slabs([(r0, r1, n) for r0, r1, _ in slabs], C, N, T, 1 << 30)
    assert any(int(wide[r0:r1, r1:].sum()) > 0 for r0, r1, _ in slabs)
    with pytest.raises(AssertionError):
        sr.check_slabs([(r0, r1, r0) for r0, r1, _ in slabs], C, N, T, 1 << 30)


def test_slab_examples():
    # 40 blocks per slab, 2 classes of 9 samples: six ranges of samples, the second ending with its class (ragged)
    assert ext._seq_linear_plan(2, 9, 3, 5, 4, workspace_bytes=2 * 1440, kappa=0.0)["slabs"] == [(0, 6, 6), (6, 9, 9), (9, 12, 12), (12, 14, 14), (14, 16, 16), (16, 18, 18)]
    # 4 classes of 3 samples, 60 blocks: two classes (6 x 6 = 36; a third class would be 81), one (3 x 9; two would be 72), one (3 x 12)
    assert ext._seq_linear_plan(4, 3, 2, 5, 4, workspace_bytes=2 * 4 * 4 * 60, kappa=0.0)["slabs"] == [(0, 6, 6), (6, 9, 9), (9, 12, 12)]
    assert ext._seq_linear_plan(4, 3, 2, 5, 4, workspace_bytes=2 * 4 * 4 * 80, kappa=0.0)["slabs"] == [(0, 6, 6), (6, 12, 12)]
    # the smallest workspace route A accepts, one row of 18 blocks: 4 x 4 at the top, single rows from row 9 on
    slabs = ext._seq_linear_plan(2, 9, 3, 5, 4, workspace_bytes=2 * 4 * 3 * 18 * 3, kappa=0.0)["slabs"]
    assert slabs[0] == (0, 4, 4) and slabs[-9:] == [(r, r + 1, r + 1) for r in range(9, 18)]


@pytest.mark.parametrize("C,N,O,I,W,want", [(2, 4, 11, 5, 4 * 8 * 5 * 4, [(0, 4), (4, 8), (8, 11)]), (2, 4, 11, 5, 1 << 30, [(0, 11)]),
                                            (2, 4, 11, 5, 1, [(o, o + 1) for o in range(11)]), (2, 4, 12, 5, 4 * 8 * 5 * 4, [(0, 4), (4, 8), (8, 12)]),
                                            (10, 64, 3072, 768, 256 * MIB, None)])
def test_chunks(C, N, O, I, W, want):
    """A chunk of the factor and the scratch buffer of its SYRK share the workspace; ``want``: the chunks with a SYRK that takes
    none, otherwise the library's own query."""
    ws = (lambda n, p: 0) if want is not None else kernels.gram_syrk_workspace_bytes
    plan = ext._seq_linear_plan(C, N, 6, O, I, workspace_bytes=W, kappa=1e30, syrk_workspace=ws)
    assert plan["route"] == "B" and plan["slabs"] == []
    sr.check_chunks(plan["chunks"], C, N, O, I, W, ws)
    if want is not None:
        assert plan["chunks"] == want
    else:
        step = plan["chunks"][0][1]
        assert step > 1 and plan["chunks"][-1][1] - plan["chunks"][-1][0] <= step
        assert plan["chunks"] == ext._seq_linear_plan(C, N, 6, O, I, kappa=1e30)["chunks"]     # the default query is the library's


def test_chunks_shrink_for_the_scratch_buffer_of_the_syrk():
    C, N, O, I, W = 2, 4, 64, 5, 4 * 8 * 5 * 40
    ws = lambda n, p: 6 * n * p                                                           # noqa: E731  (1.5 times the chunk)
    plan = ext._seq_linear_plan(C, N, 6, O, I, workspace_bytes=W, kappa=1e30, syrk_workspace=ws)
    sr.check_chunks(plan["chunks"], C, N, O, I, W, ws)
    step = plan["chunks"][0][1]
    assert 40 * 2 // 5 * 7 // 8 <= step <= 40 * 2 // 5                                    # 10 n p <= W: 16 features, reached from 40 by 7 / 8
