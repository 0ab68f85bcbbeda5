"""``kernels.gram_directions_batched`` (vivit_gram_directions_batched_f32) on the GPU.

Reference: the fp64 evaluation of the header's two formulas on the same fp32 inputs (tests/gram_directions_refs.py).  The
accuracy yardstick is not a number: the four-launch path the kernel replaces (``gemm_tn`` + ``scale_cols_rsqrt_`` +
``gemm_nn`` + ``dir_curvature``) runs on the same inputs in the same test, and the new kernel's largest error -- relative
to the largest reference entry of each output -- may be at most TWICE that path's (another summation order; the precedent
of tests/test_gram_precision_gpu.py).  Both figures are printed.  Further: a problem's bits do not depend on the batch it is
in, two runs give equal bits, eigenvalues <= 0 give the IEEE classes of the four-launch path, padded leading dimensions are
honoured (the padding is NaN), and bad arguments are refused with VIVIT_E_BADARG before anything is launched."""
import ctypes
import math

import pytest
import torch

import gram_directions_refs as R
from vivit_amd import _lib, kernels

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
DEV = torch.device("cuda:0")


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def errors(path, grams, Zts, evals, VtGs, C, N):
    """``(gamma error, lambda error)`` of ``path(b) -> (gammas, lambdas)``: the largest over the batch."""
    eg = el = 0.0
    for b, (G, Zt, w, VtG) in enumerate(zip(grams, Zts, evals, VtGs)):
        ref_g, ref_l = R.directions_fp64(G, Zt, w, VtG, C, N, **R.SCALARS)
        gam, lam = path(b)
        assert gam.shape == ref_g.shape and lam.shape == ref_l.shape
        eg, el = max(eg, R.rel_error(gam, ref_g)), max(el, R.rel_error(lam, ref_l))
    return eg, el


@pytest.mark.parametrize("batch", R.BATCHES)
@pytest.mark.parametrize("n,C,N,M", R.SHAPES, ids=[f"n{s[0]}-C{s[1]}-N{s[2]}-M{s[3]}" for s in R.SHAPES])
def test_error_at_most_twice_the_four_launch_path(n, C, N, M, batch):
    Ks = R.mixed_K(n, batch)
    grams, Zts, evals, VtGs = R.make_batch(n, M, Ks, seed=n + batch, device=DEV)
    kept = [G.clone() for G in grams]
    gammas, lambdas = kernels.gram_directions_batched(grams, Zts, evals, VtGs, C, N, **R.SCALARS)
    assert [tuple(g.shape) for g in gammas] == [(M, K) for K in Ks]
    assert [tuple(l.shape) for l in lambdas] == [(N, K) for K in Ks]
    assert all(torch.equal(a, b) for a, b in zip(grams, kept)), "the Gram matrices are read, not destroyed"
    new = errors(lambda b: (gammas[b], lambdas[b]), grams, Zts, evals, VtGs, C, N)
    old = errors(lambda b: R.four_launch(kernels, grams[b], Zts[b], evals[b], VtGs[b], C, N, **R.SCALARS)
                 if Ks[b] else (gammas[b], lambdas[b]), grams, Zts, evals, VtGs, C, N)
    print(f"\n  n={n} C={C} N={N} M={M} batch={batch} K={Ks}: gammas batched {new[0]:.3e} four-launch {old[0]:.3e}; "
          f"lambdas batched {new[1]:.3e} four-launch {old[1]:.3e}")
    assert new[0] <= 2.0 * old[0], f"gammas: {new[0]:.3e} > 2 x {old[0]:.3e}"
    assert new[1] <= 2.0 * old[1], f"lambdas: {new[1]:.3e} > 2 x {old[1]:.3e}"


@pytest.mark.parametrize("n,C,N,M", [R.SHAPES[1], R.SHAPES[3], R.SHAPES[4]], ids=["n12", "n320", "n1280"])
def test_batch_independence_and_determinism(n, C, N, M):
    Ks = R.mixed_K(n, 11)
    grams, Zts, evals, VtGs = R.make_batch(n, M, Ks, seed=7, device=DEV)
    gam11, lam11 = kernels.gram_directions_batched(grams, Zts, evals, VtGs, C, N, **R.SCALARS)
    again_g, again_l = kernels.gram_directions_batched(grams, Zts, evals, VtGs, C, N, **R.SCALARS)
    for b in range(11):
        assert same_bits(gam11[b], again_g[b]) and same_bits(lam11[b], again_l[b]), f"problem {b}: two runs differ"
        g1, l1 = kernels.gram_directions_batched([grams[b]], [Zts[b]], [evals[b]], [VtGs[b]], C, N, **R.SCALARS)
        assert same_bits(gam11[b], g1[0]) and same_bits(lam11[b], l1[0]), f"problem {b} alone differs from the batch of 11"
    # ... and in other company, at another place of the batch
    order = [10, 3, 0]
    g3, l3 = kernels.gram_directions_batched([grams[b] for b in order], [Zts[b] for b in order], [evals[b] for b in order],
                                             [VtGs[b] for b in order], C, N, **R.SCALARS)
    for pos, b in enumerate(order):
        assert same_bits(gam11[b], g3[pos]) and same_bits(lam11[b], l3[pos])


def test_more_problems_than_one_launch_carries():
    """The descriptors travel as kernel arguments, 64 per launch: 70 problems take the second launch as well."""
    n, C, N, M = R.SHAPES[1]
    Ks = [(3 * b) % (n + 1) for b in range(70)]
    grams, Zts, evals, VtGs = R.make_batch(n, M, Ks, seed=11, device=DEV)
    gammas, lambdas = kernels.gram_directions_batched(grams, Zts, evals, VtGs, C, N, **R.SCALARS)
    for b in (0, 1, 63, 64, 69):
        g1, l1 = kernels.gram_directions_batched([grams[b]], [Zts[b]], [evals[b]], [VtGs[b]], C, N, **R.SCALARS)
        assert same_bits(gammas[b], g1[0]) and same_bits(lambdas[b], l1[0])
    new = errors(lambda b: (gammas[b], lambdas[b]), grams, Zts, evals, VtGs, C, N)
    assert max(new) < 1e-5


def test_zero_and_negative_eigenvalues_give_the_four_launch_classes():
    """1 / sqrt(0) = inf, 1 / sqrt(-1) = NaN, x / 0 = inf, 0 / 0 = NaN: as ``scale_cols_rsqrt_`` and ``dir_curvature``."""
    n, C, N, M = 12, 3, 4, 5
    (G,), (Zt,), (w,), (VtG,) = R.make_batch(n, M, [6], seed=3, device=DEV)
    w[1], w[3], w[4] = 0.0, -1.0, 0.0
    Zt[4] = 0.0                      # direction 4: 0 * inf in gammas, 0 / 0 in lambdas
    VtG[:, 2] = 0.0                  # column 2 of gammas: 0 * inf for direction 1
    (gam,), (lam,) = kernels.gram_directions_batched([G], [Zt], [w], [VtG], C, N, **R.SCALARS)
    ref_g, ref_l = R.four_launch(kernels, G, Zt, w, VtG, C, N, **R.SCALARS)

    def classes(t):
        c = torch.zeros(t.shape, dtype=torch.int32, device=t.device)
        c[t.isnan()], c[t == float("inf")], c[t == float("-inf")] = 2, 1, -1
        return c.cpu()

    assert torch.equal(classes(gam), classes(ref_g)) and torch.equal(classes(lam), classes(ref_l))
    assert bool(gam[:, 3].isnan().all()) and bool((lam[:, 3] < 0).all())           # negative eigenvalue
    assert bool(gam[:, 4].isnan().all()) and bool(lam[:, 4].isnan().all())         # 0 * inf, 0 / 0
    assert math.isnan(float(gam[2, 1])) and bool(gam[[0, 1, 3, 4], 1].isinf().all())
    assert bool((lam[:, 1] == float("inf")).all())
    fine = [0, 2, 5]
    assert bool(gam[:, fine].isfinite().all()) and bool(lam[:, fine].isfinite().all())


def raw(grams, Zts, evals, VtGs, gammas, lambdas, Ks, n, ldg, ldz, ldv, C, N, M, batch=None, null=()):
    """The C entry point itself.  ``null``: names of the host arrays to pass as NULL."""
    B = len(Ks) if batch is None else batch

    def arr(ts, name):
        if name in null:
            return None
        return (ctypes.c_void_p * len(ts))(*[(t.data_ptr() if t is not None and t.numel() else None) for t in ts])

    k_arr = None if "K" in null else (ctypes.c_int64 * len(Ks))(*Ks)
    return _lib.load().vivit_gram_directions_batched_f32(
        arr(grams, "G"), B, n, ldg, arr(Zts, "Zt"), ldz, arr(evals, "evals"), arr(VtGs, "VtG"), ldv, k_arr, C, N, M,
        R.SCALARS["alpha_gram"], R.SCALARS["alpha_gamma"], R.SCALARS["lambda_scale"], arr(gammas, "gammas"),
        arr(lambdas, "lambdas"), torch.cuda.current_stream(DEV).cuda_stream)


def padded(t, ld):
    buf = torch.full((t.shape[0], ld), float("nan"), device=t.device)
    buf[:, : t.shape[1]] = t
    return buf


@pytest.mark.parametrize("n,C,N,M", [R.SHAPES[1], R.SHAPES[2], R.SHAPES[3]], ids=["n12", "n193", "n320"])
def test_padded_leading_dimensions(n, C, N, M):
    Ks = R.mixed_K(n, 8)
    grams, Zts, evals, VtGs = R.make_batch(n, M, Ks, seed=5, device=DEV)
    want_g, want_l = kernels.gram_directions_batched(grams, Zts, evals, VtGs, C, N, **R.SCALARS)
    ldg, ldz, ldv = n + 3, n + 5, M + 1
    pg, pz, pv = [padded(G, ldg) for G in grams], [padded(Z, ldz) for Z in Zts], [padded(V, ldv) for V in VtGs]
    gammas = [torch.full((M, K), float("nan"), device=DEV) for K in Ks]
    lambdas = [torch.full((N, K), float("nan"), device=DEV) for K in Ks]
    assert raw(pg, pz, evals, pv, gammas, lambdas, Ks, n, ldg, ldz, ldv, C, N, M) == _lib.VIVIT_OK
    for b in range(8):
        assert same_bits(gammas[b], want_g[b]) and same_bits(lambdas[b], want_l[b]), f"problem {b}"
    # the launcher keeps operands that share a leading dimension as they are, and copies the rest
    views_g, views_l = kernels.gram_directions_batched([p[:, :n] for p in pg], [p[:, :n] for p in pz], evals,
                                                       [p[:, :M] for p in pv], C, N, **R.SCALARS)
    mixed_g, mixed_l = kernels.gram_directions_batched([pg[0][:, :n]] + grams[1:], Zts, evals, VtGs, C, N, **R.SCALARS)
    for b in range(8):
        assert same_bits(views_g[b], want_g[b]) and same_bits(views_l[b], want_l[b])
        assert same_bits(mixed_g[b], want_g[b]) and same_bits(mixed_l[b], want_l[b])


def test_bad_arguments_are_refused_and_nothing_is_written():
    """Every refused call gets pointers to full-sized operands: even a call that slipped through would stay in bounds."""
    n, C, N, M = 12, 3, 4, 5
    Ks = [3, 0, 12]
    grams, Zts, evals, VtGs = R.make_batch(n, M, Ks, seed=9, device=DEV)
    gammas = [torch.full((M, n), -7.0, device=DEV) for _ in Ks]      # room for K = n each
    lambdas = [torch.full((N, n), -7.0, device=DEV) for _ in Ks]
    ok = dict(grams=grams, Zts=Zts, evals=evals, VtGs=VtGs, gammas=gammas, lambdas=lambdas, Ks=Ks, n=n, ldg=n, ldz=n, ldv=M,
              C=C, N=N, M=M)
    bad = [
        dict(batch=-1), dict(n=-12), dict(C=-3, N=-4), dict(M=-1), dict(C=2), dict(N=5), dict(ldg=n - 1), dict(ldz=n - 1),
        dict(ldv=M - 1), dict(Ks=[3, -1, 12]), dict(Ks=[3, 0, 13]),
        dict(null=("G",)), dict(null=("Zt",)), dict(null=("evals",)), dict(null=("VtG",)), dict(null=("K",)),
        dict(null=("gammas",)), dict(null=("lambdas",)),
        dict(grams=[grams[0], None, None]), dict(Zts=[Zts[0], None, None]), dict(evals=[None, None, evals[2]]),
        dict(VtGs=[None, None, VtGs[2]]), dict(gammas=[gammas[0], None, None]), dict(lambdas=[None, None, lambdas[2]]),
    ]
    for change in bad:
        assert raw(**{**ok, **change}) == _lib.VIVIT_E_BADARG, change
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in gammas + lambdas), "a refused call wrote something"
    # what is legal: an empty batch, K = 0 with that problem's pointers NULL, M = 0
    assert raw(**{**ok, "batch": 0}) == _lib.VIVIT_OK
    assert raw(**{**ok, "grams": [grams[0], None, grams[2]], "VtGs": [VtGs[0], None, VtGs[2]],
                  "gammas": [gammas[0], None, gammas[2]], "lambdas": [lambdas[0], None, lambdas[2]]}) == _lib.VIVIT_OK
    torch.cuda.synchronize()
    assert bool((gammas[1] == -7.0).all()) and bool((lambdas[1] == -7.0).all())
    ref_g, ref_l = R.directions_fp64(grams[0], Zts[0], evals[0], VtGs[0], C, N, **R.SCALARS)
    assert R.rel_error(gammas[0].flatten()[: M * 3].view(M, 3), ref_g) < 1e-5
    assert R.rel_error(lambdas[0].flatten()[: N * 3].view(N, 3), ref_l) < 1e-5


def test_launcher_refuses_mixed_batches():
    n, C, N, M = 12, 3, 4, 5
    grams, Zts, evals, VtGs = R.make_batch(n, M, [2, 3], seed=1, device=DEV)
    with pytest.raises(ValueError):
        kernels.gram_directions_batched(grams, Zts[:1], evals, VtGs, C, N, **R.SCALARS)
    with pytest.raises(ValueError):
        kernels.gram_directions_batched([grams[0], grams[1][:8, :8]], Zts, evals, VtGs, C, N, **R.SCALARS)
    with pytest.raises(ValueError):
        kernels.gram_directions_batched(grams, Zts, evals, [VtGs[0], VtGs[1][:, :3]], C, N, **R.SCALARS)
    with pytest.raises(ValueError):
        kernels.gram_directions_batched([], [], [], [], C, N, **R.SCALARS)
    with pytest.raises(RuntimeError):
        kernels.gram_directions_batched([G.cpu() for G in grams], Zts, evals, VtGs, C, N, **R.SCALARS)
