"""Host checks of tests/eig_edge_refs.py (no GPU): every input of the scale ladder and every degenerate input goes through
tests/helpers.py::OracleBackend -- fp64 LAPACK, rounded to fp32 -- and through ``check_eigen``, which shows that each bound
the GPU tests assert is met by a correctly rounded answer at that input; the power-of-two shifts are exact where they are
said to be; and ``check_eigen`` rejects planted errors."""
import numpy as np
import pytest
import torch

import eig_edge_refs as R
from helpers import OracleBackend

SIZES = (2, 33, 192, 200, 516)          # the sizes of tests/test_symeig_scale_gpu.py
LADDER = list(R.RUNGS) + ["denormal"]


def oracle_pairs(A32):
    """fp64 eigenpairs rounded to fp32, through both oracle entry points."""
    ob = OracleBackend()
    w, Z = ob.symeig(A32.double(), eigenvectors=True)
    plan = ob.symeig_reduce(A32.double())
    assert torch.equal(plan.evals, w)
    return w.float(), Z.float(), plan


def run_oracle(A32):
    n = A32.shape[0]
    small = n <= R.SMALL_N_MAX
    w, Z, plan = oracle_pairs(A32)
    if n <= 200:   # (the values-only entry: one more fp64 solve)
        R.check_eigen(A32, ob_values(A32), small=small)
    R.check_eigen(A32, w, Z, small=small)
    keep = sorted(set(list(range(max(n - 10, 0), n)) + [n // 2]))
    R.check_eigen(A32, w, plan.select(keep).float(), rows=keep, small=small)
    lo, hi = n // 3, max(2 * n // 3, n // 3 + 1)
    R.check_eigen(A32, w, Z[:, lo:hi], rows=range(lo, hi), small=small)


def ob_values(A32):
    return OracleBackend().symeig(A32.double(), eigenvectors=False)[0].float()


@pytest.mark.parametrize("rung", LADDER, ids=str)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_bounds_are_met_by_the_rounded_fp64_answer(kind, n, rung):
    run_oracle(R.scaled_case(kind, n, rung))


@pytest.mark.parametrize("n", SIZES)
def test_norm126_is_met_by_the_rounded_fp64_answer(n):
    A = R.norm126(n)
    run_oracle(A)
    norm2 = float(np.abs(R.reference(A)[1]).max())
    assert abs(np.log2(norm2) - R.NORM126_LOG2) < 1e-5 and float(A.abs().max()) < 3.0e38


@pytest.mark.parametrize("log2s", [0, -100])
@pytest.mark.parametrize("n", (33, 192, 200, 260))
@pytest.mark.parametrize("kind", R.DEGENERATE)
def test_degenerate_inputs_are_met_by_the_rounded_fp64_answer(kind, n, log2s):
    A = R.degenerate(kind, n, log2s)
    assert torch.equal(A, A.T)
    run_oracle(A)
    if log2s:
        assert torch.equal(A.double() * 2.0 ** -log2s, R.degenerate(kind, n).double())


def test_degenerate_inputs_are_what_they_say():
    n = 200
    w = lambda k: R.reference(R.degenerate(k, n))[1]   # noqa: E731
    assert not R.degenerate("zero", n).any()
    assert np.all(w("identity3") == 3.0)
    d = R.degenerate("diag_desc", n).diagonal()
    assert bool((d[:-1] > d[1:]).all())
    W = R.degenerate("tridiag_wilkinson", n)
    assert not torch.triu(W, 2).any() and bool((W.diagonal(1) == 1).all())
    B = R.degenerate("blockdiag", n)
    assert not B[: n // 3, n // 3:].any() and bool(B[: n // 3, : n // 3].all()) and bool(B[n // 3:, n // 3:].all())
    D = R.degenerate("dead_sample", n)
    assert not D[n // 2].any() and not D[:, n // 2].any() and bool(D[n // 2 + 1].any())
    assert int((np.abs(w("rank1")) > 1e-6 * np.abs(w("rank1")).max()).sum()) == 1
    assert w("neg_lowrank").min() < -100 and w("neg_lowrank").max() < 1e-4
    assert np.abs(np.abs(w("antidiag")) - 1).max() < 1e-12 and int((w("antidiag") > 0).sum()) == n // 2
    Aw = R.degenerate("arrowhead", n)
    assert not Aw[1:, 1:].triu(1).any() and bool((Aw[0, 1:] == 1).all())


# ---- the shifts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_rungs_land_where_the_table_says_and_exactly(kind, n):
    base = R.scaled(kind, n, 0)
    for rung in R.RUNGS:
        A, log2s = R.on_rung(kind, n, rung)
        amax = float(A.abs().max())
        if rung < 0:
            assert 2.0 ** rung <= amax < 2.0 ** (rung + 1)
        elif rung > 0:
            assert 2.0 ** (rung - 1) < amax <= 2.0 ** rung
        else:
            assert log2s == 0 and torch.equal(A, base)
        # which side of ssyev's window and of the solver's (sigma = 1 exactly on the unscaled rungs)
        assert (2.0 ** -51 <= amax <= 2.0 ** 51) == (rung in R.SSYEV_RUNGS), (rung, amax)
        assert (R.RMIN <= amax <= R.RMAX) == (rung in R.UNSCALED_RUNGS), (rung, amax)
        back = A.double() * 2.0 ** -log2s
        if rung == -120:   # the small entries leave the normal range: rounded to multiples of 2^-149
            assert float((back - base.double()).abs().max()) <= 2.0 ** (-150 - log2s)
            if kind in ("lowrank", "decay") and n > 2:
                assert bool(((A != 0) & (A.abs() < R.FLT_MIN_NORMAL)).any()), "no denormal entry"
        else:
            assert torch.equal(back, base.double()), rung
    A = R.denormal(kind, n)
    assert 2.0 ** -130 <= float(A.abs().max()) < 2.0 ** -129 and float(A.abs().max()) < R.FLT_MIN_NORMAL


@pytest.mark.parametrize("rung", [-50, 50])
@pytest.mark.parametrize("n", [65, 500])
@pytest.mark.parametrize("kind", ["random", "wilkinson", "clustered", "decoupled", "graded"])
def test_tridiagonal_shifts_are_exact(kind, n, rung):
    d0, e0 = R.tridiag_case(kind, n)
    d, e = R.scaled_tridiag(kind, n, rung)
    amax = max(np.abs(d).max(), np.abs(e).max())
    assert 2.0 ** -51 <= amax <= 2.0 ** 51
    s = R.shift_to_rung(max(np.abs(d0).max(), np.abs(e0).max()), rung)
    assert np.array_equal(d.astype(np.float64) * 2.0 ** -s, d0) and np.array_equal(e.astype(np.float64) * 2.0 ** -s, e0)


# ---- planted errors -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 200])
def test_check_eigen_rejects_planted_errors(n):
    small = n <= R.SMALL_N_MAX
    for rung in (-100, 0, 100):
        A, _ = R.on_rung("dense", n, rung)
        w, Z, _ = oracle_pairs(A)
        R.check_eigen(A, w, Z, small=small)
        with pytest.raises(AssertionError, match="eigenvalues"):
            R.check_eigen(A, w * (1 + 1e-4), small=small)
        Zs = Z.clone()
        Zs[:, [3, n - 2]] = Z[:, [n - 2, 3]]
        with pytest.raises(AssertionError, match="residual"):
            R.check_eigen(A, w, Zs, small=small)
        with pytest.raises(AssertionError, match="orthonormality"):
            R.check_eigen(A, w, Z * (1 + 1e-4), small=small)
    # sigma undone twice at amax = 2^-100, and not at all
    A, _ = R.on_rung("lowrank", n, -100)
    w, Z, _ = oracle_pairs(A)
    sigma = 2.0 ** (1 - np.frexp(float(A.abs().max()))[1])
    for bad in (w / float(sigma), w * float(sigma)):
        assert bool(torch.isfinite(bad).all())
        with pytest.raises(AssertionError, match="eigenvalues"):
            R.check_eigen(A, bad, small=small)
    # the special structures: an eigenvalue of c I one ulp off, a diagonal entry two ulps off
    I3 = R.degenerate("identity3", n)
    w3 = torch.full((n,), 3.0)
    R.check_eigen(I3, w3, torch.eye(n), small=small)
    w3[-1] = float(np.nextafter(np.float32(3.0), np.float32(4.0)))
    with pytest.raises(AssertionError, match="exact"):
        R.check_eigen(I3, w3, small=small)
    Dg = R.degenerate("diag_desc", n)
    wd = torch.arange(1, n + 1, dtype=torch.float32)
    R.check_eigen(Dg, wd, torch.flip(torch.eye(n), [1]), small=small)
    wd[0] += 3 * R.ulp32(n)
    with pytest.raises(AssertionError, match="diagonal"):
        R.check_eigen(Dg, wd, small=small)
    with pytest.raises(AssertionError, match="non-finite"):
        R.check_eigen(Dg, torch.full((n,), float("nan")), small=small)
