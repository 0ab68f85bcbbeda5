"""fp64 references, derived error bounds and case lists for the Linear-on-sequence rule: the kernel of csrc/seq_linear.hip
(``kernels.gram_seq_reduce``) and the closures ``_linear_seq_weight_closures`` of vivit_amd/backend/extensions.py.  TEST
INFRASTRUCTURE shared by tests/test_seq_linear_refs_host.py, test_seq_linear_kernels_gpu.py and test_seq_linear_closures_gpu.py; in the
manner of tests/embedding_refs.py.

Notation of include/vivit_hip.h: ``s [C, N, T, O]`` the factor at the module output, ``z [N, T, I]`` the input, ``s' = [C N T, O]``,
``z' = [N T, I]``, ``Gs = s' s'^T``, ``Gz = z' z'^T``, ``V_t[c,n,o,i] = sum_t s[c,n,t,o] z[n,t,i]`` and
``G[(c,n),(e,m)] = sum_{t,u} Gs[(c,n,t),(e,m,u)] Gz[(n,t),(m,u)] = <V_t[c,n], V_t[e,m]>``.

Error bounds (u = 2^-24, elementwise against the fp64 reference; derived, not fitted).  gamma_k = k u / (1 - k u) bounds any sum in
which a term passes through at most k roundings, in any order, fused or not (Higham, Accuracy and Stability of Numerical Algorithms,
section 3.1), relative to the same formula on absolute values.  tau(p) = 2e-6 sqrt(p) + 1e-6 is the project's contract for a GEMM /
SYRK with contraction length p: max |error| <= tau(p) max |exact product| (tests/test_kernels_gpu.py).

* kernel   a term passes through one product, at most T^2 - 1 additions, the scaling by alpha and the beta term: k = T^2 + 3.
* route A  Gs and Gz come from the SYRK / GEMM routes: |dGs| <= tau(O) max|Gs|, |dGz| <= tau(I) max|Gz|; the T^2 terms of an entry
           then err by T^2 (tau(O) + tau(I) + tau(O) tau(I)) max|Gs| max|Gz|, plus the kernel's own gamma_k sum|terms|.  Loose by
           construction: it catches wiring errors, not rounding.
* route B  the chunk of the factor comes from the 1 x 1 convolution rule (contraction T): |dV| <= tau(T) max|V|; the SYRK of a chunk
           (contraction (o1 - o0) I <= O I) errs by tau(.) max|G_chunk| <= tau(.) max|G| (a chunk's Gram matrix is positive
           semi-definite and the chunks add up to G, so its largest entry, a diagonal one, is below G's), and adds one rounded
           accumulation: chunks (tau(step I) + 2 u) max|G| + O I (2 tau(T) + tau(T)^2) max|V|^2.
* V_mat_prod    U = class_contract (C products, C - 1 additions: gamma_{C+1} on sum|terms|), then the GEMM with z' (contraction N T).
* V_t_mat_prod  U = GEMM of mat with z' (contraction I), then class_expand (O terms) and the sum over t: gamma_{O+T+1}.
"""
import math

import torch

from epilogue_refs import EPS, F64, SENTINEL, gen, generic, misaligned, padding_untouched, with_sentinel_padding, within   # noqa: F401

# ---- tiling of csrc/seq_linear.hip as built -------------------------------------------------------------------------------------
BLOCK = 256           # lanes per workgroup (SR_BLOCK)
SPAN = 1024           # columns (e, m, u) per workgroup, at most (SR_SPAN); four per lane
ROWS_PER_GROUP = 1    # one output row (c, n) per workgroup
T_MAX = 1024          # SR_T_MAX


def outputs_per_group(T):
    """Outputs (e, m) per workgroup (sr_outputs): SPAN // T, rounded down to a multiple of 4 / gcd(T, 4) when it is at least that."""
    jt = SPAN // T
    q = 4 // math.gcd(T, 4)
    return jt - jt % q if jt >= q else jt


def gamma(k):
    return k * EPS / (1 - k * EPS)


def tau(p):
    return 2e-6 * math.sqrt(p) + 1e-6


# ---- the kernel -----------------------------------------------------------------------------------------------------------------
def seq_reduce(Gz, Gs, Cr, Nr, Cc, Nc, T, alpha=1.0, beta=0.0, G0=None):
    """(G [Cr Nr, Cc Nc] fp64, its bound).  ``Gz [Nr T, Nc T]``, ``Gs [Cr Nr T, Cc Nc T]``; ``G0`` is not read when beta == 0."""
    z = Gz.to(F64).reshape(1, Nr, T, 1, Nc, T)
    s = Gs.to(F64).reshape(Cr, Nr, T, Cc, Nc, T)
    G = alpha * (z * s).sum((2, 5)).reshape(Cr * Nr, Cc * Nc)
    mag = abs(alpha) * (z.abs() * s.abs()).sum((2, 5)).reshape(Cr * Nr, Cc * Nc)
    if beta != 0.0:
        G, mag = G + beta * G0.to(F64), mag + abs(beta) * G0.to(F64).abs()
    return G, gamma(T * T + 3) * mag


def seq_reduce_fp32(Gz, Gs, Cr, Nr, Cc, Nc, T, alpha=1.0, beta=0.0, G0=None):
    """A plain fp32 evaluation on the CPU (torch's own summation order): what correct arithmetic measures against the bound."""
    z = Gz.float().reshape(1, Nr, T, 1, Nc, T)
    s = Gs.float().reshape(Cr, Nr, T, Cc, Nc, T)
    G = torch.tensor(alpha, dtype=torch.float32) * (z * s).sum((2, 5)).reshape(Cr * Nr, Cc * Nc)
    return G + torch.tensor(beta, dtype=torch.float32) * G0.float() if beta != 0.0 else G


def make_kernel_case(seed, Cr, Nr, Cc, Nc, T):
    """(Gz, Gs, G0): generic operands, entries over three decades (CPU fp32)."""
    g = gen(seed)
    return generic(g, Nr * T, Nc * T), generic(g, Cr * Nr * T, Cc * Nc * T), generic(g, Cr * Nr, Cc * Nc)


KERNEL_T = (1, 2, 3, 5, 7, 16, 17, 63, 64, 65, 130)
KERNEL_BLOCKS = ((1, 1, 1, 1), (2, 3, 3, 5), (3, 7, 2, 4))
# (T, Cr, Nr, Cc, Nc): more than two workgroups along both axes of the grid with a ragged last span: rows are one per workgroup,
# the columns Cc Nc = 2 outputs_per_group(T) + a remainder.  Nc T is a multiple of 4 in the first three (the float4 body with
# contiguous, aligned operands) and odd in the last (the scalar body, the remainder no multiple of 4 columns)
PAST_FIRST = ((65, 2, 2, 7, 4), (16, 1, 3, 3, 47), (130, 1, 3, 1, 14), (5, 3, 1, 7, 59))


# ---- the closures ---------------------------------------------------------------------------------------------------------------
class Problem:
    """``s [C, N, *A, O]``, ``z [N, *A, I]`` (CPU fp32) and the fp64 quantities the references share, computed once."""

    def __init__(self, s, z):
        self.s, self.z = s, z
        self.C, self.N, self.O, self.I = s.shape[0], s.shape[1], s.shape[-1], z.shape[-1]
        C, N, O, I = self.C, self.N, self.O, self.I
        self.s4 = s.to(F64).reshape(C, N, -1, O)
        self.T = T = self.s4.shape[2]
        self.z3 = z.to(F64).reshape(N, T, I)
        self.V = torch.einsum("cnto,nti->cnoi", self.s4, self.z3)               # the explicit factor
        self.G = self.V.reshape(C * N, O * I) @ self.V.reshape(C * N, O * I).T
        s2, z2 = self.s4.reshape(C * N * T, O), self.z3.reshape(N * T, I)
        self.Gs, self.Gz = s2 @ s2.T, z2 @ z2.T

    def gram_expanded(self):
        """The identity of the rule, in fp64: (G from Gs and Gz, sum|terms|)."""
        C, N, T = self.C, self.N, self.T
        return seq_reduce(self.Gz, self.Gs, C, N, C, N, T)[0], seq_reduce(self.Gz.abs(), self.Gs.abs(), C, N, C, N, T)[0]

    def bound_A(self):
        T, O, I = self.T, self.O, self.I
        wiring = T * T * (tau(O) + tau(I) + tau(O) * tau(I)) * self.Gs.abs().max() * self.Gz.abs().max()
        return wiring + gamma(T * T + 3) * self.gram_expanded()[1]

    def bound_B(self, chunks, step):
        T, O, I = self.T, self.O, self.I
        return (chunks * (tau(step * I) + 2 * EPS) * self.G.abs().max() + O * I * (2 * tau(T) + tau(T) ** 2) * self.V.abs().max() ** 2
                ).expand_as(self.G)

    def prior_bound(self, G0, beta):
        """What a prior ``G0`` adds to either bound: one product and one addition."""
        return gamma(2) * abs(beta) * G0.to(F64).abs()

    def vmp(self, mat):
        """``mat [F, C, N]`` -> (out [F, O, I] fp64, bound)."""
        m = mat.to(F64)
        out = torch.einsum("fcn,cnoi->foi", m, self.V)
        U_abs = torch.einsum("fcn,cnto->font", m.abs(), self.s4.abs())
        mag = torch.einsum("font,nti->foi", U_abs, self.z3.abs())
        rounding = gamma(self.C + 1) * mag
        return out, tau(self.N * self.T) * (out.abs().max() + rounding.max()) + rounding

    def vtmp(self, mat):
        """``mat [F, O, I]`` -> (out [F, C, N] fp64, bound)."""
        m = mat.to(F64)
        out = torch.einsum("foi,cnoi->fcn", m, self.V)
        U = torch.einsum("foi,nti->font", m, self.z3)
        dU = tau(self.I) * U.abs().max()
        s_abs = self.s4.abs()
        return out, dU * s_abs.sum((2, 3)).unsqueeze(0) + gamma(self.O + self.T + 1) * torch.einsum("cnto,font->fcn", s_abs, U.abs() + dU)


def make_problem(seed, C, N, A, O, I):
    """``A``: the tuple of extra dimensions, T = prod(A)."""
    g = gen(seed)
    return Problem(generic(g, C, N, *A, O), generic(g, N, *A, I))


# (C, N, T, O, I) of the host identity check: T = 1, odd sizes, O or I = 1, T above O and I
IDENTITY_SHAPES = ((1, 1, 1, 1, 1), (3, 5, 4, 6, 7), (2, 9, 3, 5, 4), (2, 4, 6, 11, 5), (2, 3, 1, 4, 5), (3, 2, 7, 1, 3), (2, 3, 5, 4, 1),
                   (2, 2, 17, 3, 2))


# ---- the planner ----------------------------------------------------------------------------------------------------------------
def check_slabs(slabs, C, N, T, W):
    """The slabs ``(r0, r1, cols)`` of a route-A plan: rows in order, contiguous, covering 0 .. C N; each a range of whole classes
    or of samples of one class; the columns 0 .. cols - 1 of a slab reach its diagonal and stop at its own last row (whole classes
    of columns under whole classes of rows); each block of Gs ``[(r1 - r0) T, cols T]`` within W bytes (W: half the workspace
    constant).  Returns the [C N, C N] count of how often an entry is computed, from the plan's own column ends."""
    n = C * N
    count = torch.zeros(n, n, dtype=torch.int64)
    at = 0
    for r0, r1, cols in slabs:
        assert r0 == at and r0 < r1 <= n, (slabs, r0, r1)
        whole = r0 % N == 0 and r1 % N == 0
        assert whole or (r0 // N == (r1 - 1) // N), f"slab {(r0, r1)} is neither whole classes nor within one"
        assert r1 <= cols <= n and (not whole or cols % N == 0), f"slab {(r0, r1)} has columns 0 .. {cols}"
        assert 4 * (r1 - r0) * T * cols * T <= W, f"slab {(r0, r1, cols)} needs {4 * (r1 - r0) * T * cols * T} bytes of {W}"
        count[r0:r1, :cols] += 1
        at = r1
    assert at == n
    return count


def slab_rows(slabs):
    return [(r0, r1) for r0, r1, _ in slabs]


def check_chunks(chunks, C, N, O, I, W, syrk_workspace=lambda n, p: 0):
    """The chunks of a route-B plan: in order, contiguous, covering 0 .. O; a chunk of the factor and the scratch buffer of its SYRK
    within W bytes together (or a single feature)."""
    at = 0
    for o0, o1 in chunks:
        assert o0 == at and o0 < o1 <= O
        assert 4 * C * N * (o1 - o0) * I + syrk_workspace(C * N, (o1 - o0) * I) <= W or o1 - o0 == 1
        at = o1
    assert at == O
