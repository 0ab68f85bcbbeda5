"""fp64 reference and inputs for ``vivit_gram_directions_batched_f32`` (tests/test_gram_directions_batched_gpu.py).

The reference evaluates the two formulas of include/vivit_hip.h on the SAME fp32 inputs in fp64:

  gammas[j, k]  = alpha_gamma * sum_i VtG[i, j] Zt[k, i] / sqrt(evals[k])
  lambdas[m, k] = lambda_scale * sum_c (alpha_gram * sum_i G[(c, m), i] Zt[k, i])^2 / evals[k]

(vivit/optim/directional_damped_newton.py:342,348-351 with the scalings folded in).  The yardstick of the accuracy test is
the four-launch path the kernel replaces, evaluated by :func:`four_launch` on the same inputs."""
import torch

F64 = torch.float64
# (n, C, N, M): M != N everywhere; 193 is prime (C = 1), 1280 the largest size of the batched eigensolver
SHAPES = [(1, 1, 1, 3), (12, 3, 4, 5), (193, 1, 193, 40), (320, 10, 32, 48), (1280, 10, 128, 96)]
BATCHES = [1, 8, 11]
SCALARS = dict(alpha_gram=0.64, alpha_gamma=25.6, lambda_scale=32.0)


def directions_fp64(G, Zt, evals, VtG, C, N, alpha_gram, alpha_gamma, lambda_scale):
    """``(gammas [M, K], lambdas [N, K])`` in fp64 from fp32 operands (any device)."""
    G, Zt, w, VtG = G.to(F64), Zt.to(F64), evals.to(F64), VtG.to(F64)
    K = w.numel()
    gammas = alpha_gamma * (VtG.T @ Zt.T) / w.sqrt()
    GE = alpha_gram * (G @ Zt.T)
    lambdas = lambda_scale * (GE.view(C, N, K) ** 2).sum(0) / w
    return gammas, lambdas


def four_launch(kernels, G, Zt, evals, VtG, C, N, alpha_gram, alpha_gamma, lambda_scale):
    """K5 + K6 as ``gram_space_directions`` issues them: ``gemm_tn`` + ``scale_cols_rsqrt_`` + ``gemm_nn`` + ``dir_curvature``."""
    E = Zt.T.contiguous()
    gammas = kernels.gemm_tn(VtG, E, alpha=alpha_gamma)
    kernels.scale_cols_rsqrt_(gammas, evals)
    GE = kernels.gemm_nn(G, E, alpha=alpha_gram)
    return gammas, kernels.dir_curvature(GE, evals, C, N, scale=lambda_scale)


def mixed_K(n, batch):
    """Kept directions per problem: mixed within a batch, with 0, 1 and (for the small sizes) n among them."""
    base = [10, 0, 1, 7, 16, 3, 9, 2, 12, 5, 8]
    if n <= 12:
        base = [n, 0, 1, min(n, 7), n, min(n, 3), min(n, 9), min(n, 2), n, min(n, 5), min(n, 8)]
    Ks = [min(k, n) for k in base[:batch]]
    if batch == 1:
        Ks = [min(n, 10)]
    return Ks


def make_problem(n, M, K, seed, device="cpu"):
    """One problem: a symmetric ``G`` with entries of order one, unit rows ``Zt``, eigenvalues in [0.5, 2.5), ``VtG``."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(n, n, generator=g)
    G = (A + A.T) / 2
    Zt = torch.randn(K, n, generator=g)
    Zt = Zt / Zt.norm(dim=1, keepdim=True).clamp_min(1e-30)
    evals = 0.5 + 2.0 * torch.rand(K, generator=g)
    VtG = torch.randn(n, M, generator=g)
    return [t.to(device) for t in (G, Zt, evals, VtG)]


def make_batch(n, M, Ks, seed=0, device="cpu"):
    probs = [make_problem(n, M, K, 1000 * seed + b, device) for b, K in enumerate(Ks)]
    return [list(col) for col in zip(*probs)]   # grams, Zts, evals, VtGs


def rel_error(got, ref):
    """Largest error relative to the largest reference entry of this output (0 for an empty output)."""
    if ref.numel() == 0:
        return 0.0
    return float((got.to(F64).cpu() - ref.cpu()).abs().max() / ref.abs().max())
