"""fp64 references, input builders and case lists for the epilogue and factor-rule kernels (csrc/elementwise.hip, the
reductions of csrc/jacobians.hip, the Linear rule of csrc/factors.hip).  TEST INFRASTRUCTURE: a plain module shared by
tests/test_epilogue_refs_host.py (no GPU) and tests/test_epilogue_kernels_gpu.py.

Every reference restates the formula of include/vivit_hip.h in torch fp64.  Every operation has two input families:

* exact: small integers.  Entries are drawn from {-4..4}; alpha, beta, scale, pre, mean and rstd are powers of two; evals
  are of the form 4^j.  Every product and every partial sum is then a dyadic number below 2^24 in magnitude, so the fp32
  result does not depend on the summation order or on FMA contraction and must equal the fp64 reference BIT FOR BIT
  (tests/test_epilogue_refs_host.py asserts this precondition for every case the GPU tests use).
* generic: seeded randn with magnitudes spread over three orders, compared under the derived bounds below.

Error bounds of the generic family (eps = 2^-24, elementwise against the fp64 reference; derived, not tuned):
  Hadamard (block): 4 eps (|alpha z s| + |beta g|) -- three roundings of the product chain, two of the accumulate.
  length-L sums: (L + 2) eps sum|terms| -- the worst case of any summation order.  (Loose on purpose: the exact family
    catches a dropped, duplicated or misindexed element, this one a precision regression.)
  finished BatchNorm weight rule (mx - mean msum) rstd: eps ((L + 4) sum|M x| + (L + 4) |mean| sum|M|) |rstd|.
  scale_cols_rsqrt_, scale_rows_rsqrt, the division of dir_curvature: 4 eps relative on top of the bound of the argument.
"""
import torch

EPS = 2.0 ** -24
SENTINEL = -24601.0          # finite, exactly representable, outside the range of both input families
F64 = torch.float64


# ---- input builders ---------------------------------------------------------------------------------------------------
def gen(seed):
    return torch.Generator().manual_seed(seed)


def exact(g, *shape):
    """fp32 integers from {-4..4} (CPU)."""
    return torch.randint(-4, 5, shape, generator=g).float()


def generic(g, *shape):
    """fp32 randn, each entry scaled by 10^u with u uniform in [-2, 1] (CPU)."""
    return (torch.randn(*shape, generator=g, dtype=F64) * 10.0 ** (torch.rand(*shape, generator=g, dtype=F64) * 3 - 2)).float()


def family(name, g, *shape):
    return exact(g, *shape) if name == "exact" else generic(g, *shape)


def evals_for(name, g, K):
    """Positive ``evals``: 4^j (j in -3..3) for the exact family, |randn| + 0.1 spread over three orders otherwise."""
    if name == "exact":
        return (4.0 ** torch.randint(-3, 4, (K,), generator=g).double()).float()
    return (generic(g, K).abs() + 0.01).float()


def misaligned(t):
    """A contiguous copy of ``t`` (same device) whose ``data_ptr() % 16 == 4``."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def with_sentinel_padding(rows, cols, ld, device="cpu"):
    """(``buf [rows, ld]`` filled with SENTINEL, its ``[:, :cols]`` view): a test writes through the view and asserts
    afterwards with :func:`padding_untouched` that the columns ``cols .. ld-1`` are unchanged bit for bit."""
    buf = torch.full((rows, ld), SENTINEL, dtype=torch.float32, device=device)
    return buf, buf[:, :cols]


def padding_untouched(buf, cols):
    return bool((buf[:, cols:] == SENTINEL).all())


# ---- references (fp64; arguments of any float dtype, any device) ---------------------------------------------------------
def hadamard(Gz, Gs, C, N, alpha=1.0, beta=0.0, G0=None):
    """G[c,n,d,m] = alpha Gz[n,m] Gs[c,n,d,m] + beta G0[c,n,d,m] -> [C N, C N]; G0 is not read when beta == 0."""
    return hadamard_block(Gz, Gs, C, N, C, N, alpha, beta, G0)


def hadamard_block(Gz, Gs, Cr, Nr, Cc, Nc, alpha=1.0, beta=0.0, G0=None, ldg=None):
    """G[(c,n),(d,m)] = alpha Gz[n,m] Gs[(c,n),(d,m)] + beta G0[(c,n),(d,m)] -> [Cr Nr, Cc Nc].  With ``ldg`` the result is
    the whole ``[Cr Nr, ldg]`` buffer: ``G0`` is that buffer on entry and its columns beyond ``Cc Nc`` come back unchanged."""
    rows, cols = Cr * Nr, Cc * Nc
    res = alpha * (Gz.to(F64).reshape(1, Nr, 1, Nc) * Gs.to(F64).reshape(Cr, Nr, Cc, Nc)).reshape(rows, cols)
    if ldg is None:
        return res + beta * G0.to(F64).reshape(rows, cols) if beta != 0.0 else res
    full = G0.to(F64).reshape(rows, ldg).clone()
    full[:, :cols] = res + beta * full[:, :cols] if beta != 0.0 else res
    return full


def class_contract(mat, s):
    """T[f,o,n] = sum_c mat[f,c,n] s[c,n,o]."""
    return torch.einsum("fcn,cno->fon", mat.to(F64), s.to(F64))


def class_expand(s, U):
    """R[f,c,n] = sum_o s[c,n,o] U[f,o,n]."""
    return torch.einsum("cno,fon->fcn", s.to(F64), U.to(F64))


def dir_curvature(GE, evals, C, N, scale):
    """lambdas[n,k] = scale sum_c GE[(c,n),k]^2 / evals[k] (IEEE division: x/0 = inf, 0/0 = NaN)."""
    K = evals.numel()
    return scale * (GE.to(F64).reshape(C, N, K) ** 2).sum(0) / evals.to(F64)


def scale_cols_rsqrt(X, evals, pre=1.0):
    """X[r,k] pre / sqrt(evals[k])."""
    return X.to(F64) * (pre / evals.to(F64).sqrt())


def row_sqnorm(tensors, acc0=None):
    """acc[k] = acc0[k] + sum_t ||tensors[t][k]||^2."""
    K = tensors[0].shape[0]
    acc = torch.zeros(K, dtype=F64, device=tensors[0].device) if acc0 is None else acc0.to(F64).clone()
    for t in tensors:
        acc = acc + (t.to(F64).reshape(K, -1) ** 2).sum(1)
    return acc


def normalize_rows(tensors):
    """tensors[t][k] / sqrt(sum_t ||tensors[t][k]||^2), as a list."""
    K = tensors[0].shape[0]
    r = 1.0 / row_sqnorm(tensors).sqrt()
    return [t.to(F64) * r.view(K, *([1] * (t.dim() - 1))) for t in tensors]


def row_dot(M, X=None, rows_x=1):
    """out[r] = sum_l M[r,l] (X[r % rows_x, l] if X is given else 1)."""
    M = M.to(F64)
    if X is None:
        return M.sum(1)
    rows, L = M.shape
    return (M.reshape(rows // rows_x, rows_x, L) * X.to(F64).reshape(1, rows_x, L)).sum(2).reshape(rows)


def bn_eval_rules(M, x, scale, mean=None, rstd=None):
    """M [V,N,C,*sp], x [N,C,*sp], scale [C] -> (out = M scale_c, mx = sum_l M x, msum = sum_l M); with mean / rstd [C] mx
    is the finished weight rule (mx - mean_c msum) rstd_c."""
    Vd, N, C = M.shape[:3]
    Mf, xf = M.to(F64).reshape(Vd, N, C, -1), x.to(F64).reshape(1, N, C, -1)
    out = (Mf * scale.to(F64).view(1, 1, C, 1)).reshape(M.shape)
    mx, msum = (Mf * xf).sum(3), Mf.sum(3)
    if mean is not None:
        mx = (mx - mean.to(F64).view(1, 1, C) * msum) * rstd.to(F64).view(1, 1, C)
    return out, mx, msum


def symmetrize_lower(G):
    """G[i][j] = G[j][i] for j > i; the lower triangle and the diagonal as they are."""
    G = G.to(F64)
    return torch.tril(G) + torch.tril(G, -1).T


def linear_weight_mjp(s, z):
    """V[c,n,o,i] = s[c,n,o] z[n,i]."""
    return torch.einsum("cno,ni->cnoi", s.to(F64), z.to(F64))


# ---- error bounds of the generic family -----------------------------------------------------------------------------------
def sum_bound(L, mag):
    """(L + 2) eps sum|terms| for a length-L sum whose absolute terms add up to ``mag``."""
    return (L + 2) * EPS * mag


def hadamard_bound(mag):
    """4 eps (|alpha z s| + |beta g|); ``mag`` is the reference evaluated on absolute values."""
    return 4 * EPS * mag


def bn_weight_bound(L, sum_abs_mx, sum_abs_m, mean, rstd):
    C = mean.numel()
    return EPS * ((L + 4) * sum_abs_mx + (L + 4) * mean.to(F64).abs().view(1, 1, C) * sum_abs_m) * rstd.to(F64).abs().view(1, 1, C)


def within(got, ref, bound):
    """``|got - ref| <= bound`` elementwise (fp64), with the worst ratio for the failure message."""
    err = (got.to(F64) - ref.to(F64)).abs()
    bad = err > bound
    if bool(bad.any()):
        ratio = (err / bound.clamp_min(1e-300))[bad].max().item()
        return False, f"{int(bad.sum())} entries beyond the bound, worst error / bound = {ratio:.3g}"
    return True, ""


# ---- the cases of the GPU tests (shared with the host test, which checks the exactness precondition of each) -------------
# (C, N): both bodies (N % 4), (10, 256) is 6 553 600 items scalar / 1 638 400 vector: beyond ew_grid's 524 288 on both
HADAMARD_SHAPES = [(1, 1), (3, 5), (2, 8), (10, 32), (3, 7), (5, 64), (4, 129), (10, 256)]
HADAMARD_AB = [(1.0, 0.0), (2.0, 1.0), (0.25, -0.5)]
# (id, Cr, Nr, Cc, Nc): V^T g (Cc = 1) and a shard's block row (Nr < Nc); the last has 2 457 600 items (614 400 vector)
HADAMARD_BLOCK_SHAPES = [("vtg-vec", 3, 8, 1, 8), ("vtg-scalar", 3, 7, 1, 7), ("blockrow-vec", 2, 3, 2, 12),
                         ("blockrow-scalar", 2, 3, 2, 10), ("blockrow-stride", 4, 120, 4, 1280)]
# (F, C, N, O): C = 1, O = 1, N = 1, a prime N, F O N and F C N above 524 288
CLASS_SHAPES = [(2, 1, 5, 3), (3, 4, 6, 1), (2, 3, 1, 4), (3, 5, 13, 7), (6, 10, 9001, 10)]
# (C, N, K): K = 1, K prime, C = 1, N K above 524 288
DIR_CURV_SHAPES = [(3, 5, 1), (2, 6, 7), (1, 9, 4), (2, 4099, 129)]
# (rows, K, ldx): ldx in {K, K + 5}, rows = 1, above 524 288 items
SCALE_COLS_SHAPES = [(6, 4, 4), (6, 4, 9), (1, 7, 7), (1, 7, 12), (4100, 129, 134)]
# (K, per-row lengths of the tensor list): one, several and ragged chunks of 8192; K = 70 000 crosses the 65 535-row split
NORMALIZE_SHAPES = [(1, (1, 8192, 8193)), (16, (1, 8192, 8193)), (16, (3, 20000)), (1, (7,)), (16, (7,)), (70000, (3,))]
SYMM_N = [1, 2, 31, 32, 33, 64, 1000]
# (id, C, N, O, I): I % 4, O = 1, I = 1; the stride case is 20 971 520 float4 items (cap 16 777 216)
LINEAR_MJP_SHAPES = [("vec", 3, 5, 4, 8), ("scalar", 3, 5, 4, 7), ("O=1", 2, 3, 1, 12), ("I=1", 2, 3, 5, 1)]
LINEAR_MJP_STRIDE = (10, 64, 512, 256)
# row length -> body of row_dot_kernel / bn_eval_rules_kernel (L4 = L / 4 float4 per row, 64 lanes, main loop while l + 64 < L4)
# ("main|tail": some lanes are in the main loop while the others are in the tail; "main+tail": every lane ran the main loop
# and some run the tail as well)
ROW_L = {1: "scalar", 3: "scalar", 4: "vec-tail", 20: "vec-tail", 252: "vec-tail", 256: "vec-tail-full", 260: "vec-main|tail",
         400: "vec-main|tail", 508: "vec-main|tail", 512: "vec-main", 516: "vec-main+tail", 1024: "vec-main2", 1028: "vec-main2+tail",
         4100: "vec-main+tail", 257: "scalar"}
ROW_ROWS = [1, 3, 4, 5, 1000]


def make_hadamard(name, C, N, seed=0):
    g = gen(1000 * C + N + seed)
    n = C * N
    return family(name, g, N, N), family(name, g, n, n), family(name, g, n, n)


def make_hadamard_block(name, Cr, Nr, Cc, Nc, seed=0):
    g = gen(7 * Cr + 1000 * Nr + 31 * Cc + Nc + seed)
    return family(name, g, Nr, Nc), family(name, g, Cr * Nr, Cc * Nc), family(name, g, Cr * Nr, Cc * Nc)


def make_class(name, F, C, N, O):
    g = gen(F + 10 * C + 100 * N + 7 * O)
    return family(name, g, F, C, N), family(name, g, C, N, O), family(name, g, F, O, N)   # mat, s, U


def make_dir_curvature(name, C, N, K):
    g = gen(C + 10 * N + 1000 * K)
    return family(name, g, C * N, K), evals_for(name, g, K)


def make_scale_cols(name, rows, K):
    g = gen(3 * rows + K)
    return family(name, g, rows, K), evals_for(name, g, K)


def make_normalize(name, K, lens):
    g = gen(K + sum(lens))
    ts = [family(name, g, K, ln) for ln in lens]
    if name == "exact":
        ts[0][:, 0] = 1.0   # (no all-zero row: its norm would be 0)
    return ts


def make_rows(name, rows, rows_x, L):
    g = gen(rows * 10007 + L)
    return family(name, g, rows, L), family(name, g, rows_x, L)


def make_bn(name, V, N, C, L):
    g = gen(V + 10 * N + 100 * C + 1000 * L)
    M, x = family(name, g, V, N, C, L), family(name, g, N, C, L)
    if name == "exact":
        p = lambda lo, hi: (2.0 ** torch.randint(lo, hi, (C,), generator=g).double()).float()   # noqa: E731
        sign = (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()
        return M, x, p(-2, 3), p(-2, 2) * sign, p(-2, 3)
    return M, x, generic(g, C), generic(g, C), generic(g, C).abs() + 0.01   # scale, mean, rstd


def make_linear_mjp(name, C, N, O, I):
    g = gen(C + 10 * N + 100 * O + 1000 * I)
    return family(name, g, C, N, O), family(name, g, N, I)


def make_symm(n, ldg, seed=0):
    """[n, ldg] buffer: integers in the lower triangle and the diagonal, NaN in the strict upper triangle, SENTINEL padding."""
    g = gen(n + seed)
    buf, view = with_sentinel_padding(n, n, ldg)
    view.copy_(torch.randint(-1000, 1001, (n, n), generator=g).float())
    view.masked_fill_(torch.triu(torch.ones(n, n, dtype=torch.bool), 1), float("nan"))
    return buf, view


# ---- activation and pooling edges (references: torch's fp64 CPU autograd of the module itself) ---------------------------
INF, NAN = float("inf"), float("nan")
ACT_GRID = [0.0, -0.0, 1e-30, -1e-30, 1e-3, -1e-3, 1.0, -1.0, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0, 1e4, -1e4, INF, -INF, NAN]
ACT_PARAM = {"leaky_relu": 0.1, "elu": 0.7}
SELU_SCALE, SELU_ALPHA = 1.0507009873554804934193349852946, 1.6732632423543772848170429916717


def act_module(kind):
    from torch import nn

    return {"relu": nn.ReLU(), "sigmoid": nn.Sigmoid(), "tanh": nn.Tanh(), "leaky_relu": nn.LeakyReLU(0.1),
            "logsigmoid": nn.LogSigmoid(), "elu": nn.ELU(0.7), "selu": nn.SELU()}[kind]


def act_grid_input(N=4, reps=3):
    """x [N, reps * len(ACT_GRID)]: the grid tiled over a batch (fp32, CPU), every row rotated by one so that a grid value
    meets different positions of M."""
    row = torch.tensor(ACT_GRID * reps, dtype=torch.float32)
    return torch.stack([row.roll(n) for n in range(N)])


def jac_t_by_autograd(module, x, M):
    """[V, N, *out] -> [V, N, *in]: vector-Jacobian products of ``module`` at ``x`` for every slice of ``M``."""
    x = x.detach().requires_grad_(True)
    y = module(x)
    return torch.stack([torch.autograd.grad(y, x, grad_outputs=M[v], retain_graph=True)[0] for v in range(M.shape[0])])


ACT_PAD = 64


def act_reference(kind, x, M):
    """fp64 CPU autograd of the torch module: ``M [V, *x.shape] -> [V, *x.shape]``.  The operands are flattened and ACT_PAD
    benign elements are appended, so that every entry of ``x`` goes through the vectorised main loop of torch's CPU kernels
    and none through their scalar remainder loop: for ELU and SELU the two disagree on a NaN input (NaN from the vector
    loop, which computes exp(x) for every lane; the positive-side factor from the scalar one), and which entries the
    remainder holds depends on the tensor's length and the CPU's vector width."""
    V = M.shape[0]
    xp = torch.cat([x.to(F64).reshape(-1), torch.zeros(ACT_PAD, dtype=F64)])
    Mp = torch.cat([M.to(F64).reshape(V, -1), torch.zeros(V, ACT_PAD, dtype=F64)], 1)
    return jac_t_by_autograd(act_module(kind), xp, Mp)[:, :x.numel()].reshape(M.shape)


def act_derivative_fp64(kind, values):
    """f'(v) for each v by torch's fp64 CPU autograd of the module (vectorised loop, see act_reference)."""
    x = torch.tensor(values, dtype=F64)
    return act_reference(kind, x, torch.ones(1, x.numel(), dtype=F64))[0]


# (shape [N, C, H, W], kernel, stride, padding): stride larger than the kernel in both and in one dimension (input positions
# outside every window), k = s = 1, padding k // 2 with odd H and W
POOL_EDGE_GEOMS = [((3, 2, 8, 8), 2, 3, 0), ((3, 2, 7, 9), (1, 2), (2, 3), 0), ((2, 2, 5, 5), 1, 1, 0), ((2, 3, 7, 9), 3, 2, 1),
                   ((2, 2, 7, 9), 3, 1, 1)]


def pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def pool_uncovered(H, W, k, s, p):
    """bool [H, W]: True where the input position lies in no pooling window (floor mode, no dilation)."""
    (kh, kw), (sh, sw), (ph, pw) = pair(k), pair(s), pair(p)

    def cov(n, kk, ss, pp):
        on = (n + 2 * pp - kk) // ss + 1
        c = torch.zeros(n, dtype=torch.bool)
        for o in range(on):
            c[max(o * ss - pp, 0):max(min(o * ss - pp + kk, n), 0)] = True
        return c

    return ~(cov(H, kh, sh, ph).view(H, 1) & cov(W, kw, sw, pw).view(1, W))
