"""fp64 references and derived error bounds for the five kernels of the Embedding rule (csrc/embedding.hip).  TEST INFRASTRUCTURE
shared by tests/test_embedding_kernels_gpu.py; in the manner of tests/attention_refs.py.

Notation of include/vivit_hip.h: ``idx [N, T]`` token ids, ``M [V, N, T, D]`` the factor at the module output, ``W`` the vocabulary,
``Vt[v, n, w, :] = sum_{t: idx[n, t] = w} M[v, n, t, :]`` the weight factor (positions with ``idx == padding_idx`` contribute nothing).
The references are restated from ``M`` and ``idx`` in torch fp64 and never form a tensor with an axis of length ``W``: the tokens
that occur are renumbered ``0 .. Wr - 1`` first (``Wr <= N T``), which changes no sum.

Error bounds (u = 2^-24, elementwise against the fp64 reference; derived, not fitted).  An output that sums k products and additions
of fp32 numbers in ANY order, fused or not, has the error gamma_k sum|terms| at most, gamma_k = k u / (1 - k u) (Higham, Accuracy and
Stability of Numerical Algorithms, section 3.1: every term passes through at most k roundings).  sum|terms| is the same formula
evaluated on absolute values in fp64; k per output:

* compact  B[v, n, u, :]: the m rows of the slot are added, k = m (one row: a copy, and gamma_1 |x| >= 0 still holds).
* Gram     G[(v, n), (v', n')] = sum_{t, t', j} [idx[n, t] = idx[n', t']] M[v, n, t, j] M[v', n', t', j]: a term passes through the two
           compactions (at most T - 1 additions each), its product, the additions of (matched slot pairs) D products and the scaling
           by alpha: k = (matched slot pairs) D + 2 T + 2, matched slot pairs = the number of distinct tokens the two samples share.
           With beta != 0 the prior entry joins: one more product and addition, sum|terms| grows by |beta G0|.
* vmp      out[f, w, :] = sum_{v, n, t: idx[n, t] = w} mat[f, v, n] M[v, n, t, :]: compaction, product, at most V N T additions:
           k = V N T + T + 2.
* vtmp     out[f, v, n] = sum_{t, j} mat[f, idx[n, t], j] M[v, n, t, j]: compaction, product, T D additions in a lane and the lanes'
           tree (6): k = T D + T + 8.
* weight_mjp: the rows of B, copied: the bound of compact.
"""
import torch

from epilogue_refs import EPS, F64, gen, within   # noqa: F401  (re-exported for the test module)

SAMPLE_BLOCK = 16     # samples per sample block (EMB_SB of csrc/embedding.hip)


def gamma(k):
    k = torch.as_tensor(k, dtype=F64)
    return k * EPS / (1 - k * EPS)


class Case:
    """Operands (CPU, fp32 / int64) and everything the references share, computed once."""

    def __init__(self, M, idx, W, padding_idx=None):
        self.M, self.idx, self.W, self.padding_idx = M, idx, W, padding_idx
        self.V, self.N, self.T, self.D = M.shape
        V, N, T, D = M.shape
        valid = torch.ones_like(idx, dtype=torch.bool) if padding_idx is None else idx != padding_idx
        self.tokens, inv = torch.unique(idx, return_inverse=True)       # the tokens that occur, renumbered
        Wr = self.tokens.numel()
        dest = (inv + Wr * torch.arange(N).unsqueeze(1)).reshape(-1)
        Mz = M.to(F64) * valid.view(1, N, T, 1)
        self.Vt = torch.zeros(V, N * Wr, D, dtype=F64).index_add_(1, dest, Mz.reshape(V, N * T, D)).view(V, N, Wr, D)
        self.Vt_abs = torch.zeros(V, N * Wr, D, dtype=F64).index_add_(1, dest, Mz.abs().reshape(V, N * T, D)).view(V, N, Wr, D)
        self.count = torch.zeros(N * Wr, dtype=F64).index_add_(0, dest, valid.reshape(-1).to(F64)).view(N, Wr)   # rows per (n, token)
        self.present = self.count > 0
        self.Wr = Wr

    # ---- compact form
    def ids(self):
        """[N, T] int64: the distinct non-padding tokens of every sample, increasing, then -1."""
        out = torch.full((self.N, self.T), -1, dtype=torch.int64)
        for n in range(self.N):
            toks = self.tokens[self.present[n]]
            out[n, :toks.numel()] = toks
        return out

    def _to_slots(self, full):
        """[V, N, Wr, *] -> [V, N, T, *]: the rows of the present tokens in increasing order, zero rows behind."""
        out = torch.zeros(self.V, self.N, self.T, *full.shape[3:], dtype=F64)
        for n in range(self.N):
            rows = full[:, n, self.present[n]]
            out[:, n, :rows.shape[1]] = rows
        return out

    def compact(self):
        """(B [V, N, T, D] fp64, its bound)."""
        k = self._to_slots(self.count.view(1, self.N, self.Wr, 1).expand(self.V, -1, -1, -1))
        return self._to_slots(self.Vt), gamma(k) * self._to_slots(self.Vt_abs)

    # ---- Gram matrix
    def gram(self, alpha=1.0, beta=0.0, G0=None):
        """(G [V N, V N] fp64, its bound); rows v N + n."""
        n2 = self.V * self.N
        A, Aa = self.Vt.reshape(n2, -1), self.Vt_abs.reshape(n2, -1)
        G, mag = alpha * (A @ A.T), abs(alpha) * (Aa @ Aa.T)
        P = self.present.to(F64)
        k = (P @ P.T) * self.D + 2 * self.T + 2                         # [N, N]
        if beta != 0.0:
            G, mag, k = G + beta * G0.to(F64), mag + abs(beta) * G0.to(F64).abs(), k + 2
        return G, gamma(k.repeat(self.V, self.V)) * mag

    def shared_tokens(self):
        """[N, N] number of distinct tokens two samples share."""
        P = self.present.to(F64)
        return P @ P.T

    # ---- products and the explicit factor (outputs with a vocabulary axis are scattered from the renumbered one)
    def _widen(self, red, axis):
        shape = list(red.shape)
        shape[axis] = self.W
        return torch.zeros(shape, dtype=F64).index_copy_(axis, self.tokens, red)

    def vmp(self, mat):
        """``mat [F, V, N]`` -> (out [F, W, D] fp64, bound)."""
        k = self.V * self.N * self.T + self.T + 2
        red = torch.einsum("fvn,vnwd->fwd", mat.to(F64), self.Vt)
        mag = torch.einsum("fvn,vnwd->fwd", mat.to(F64).abs(), self.Vt_abs)
        return self._widen(red, 1), gamma(k) * self._widen(mag, 1)

    def vtmp(self, mat):
        """``mat [F, W, D]`` -> (out [F, V, N] fp64, bound)."""
        k = self.T * self.D + self.T + 8
        m = mat.to(F64)[:, self.tokens]
        return torch.einsum("fwd,vnwd->fvn", m, self.Vt), gamma(k) * torch.einsum("fwd,vnwd->fvn", m.abs(), self.Vt_abs)

    def factor(self):
        """(Vt [V, N, W, D] fp64, bound) -- small W only."""
        k = self.count.view(1, self.N, self.Wr, 1)
        return self._widen(self.Vt, 2), self._widen(gamma(k) * self.Vt_abs, 2)


PATTERNS = ("equal", "distinct", "random", "allpad", "onepad")


def make_case(seed, V, N, T, D, W, pattern="random", padding_idx=None):
    """Seeded operands.  ``equal``: one token everywhere; ``distinct``: no token twice in the batch (needs W >= N T); ``random``: with
    repeats; ``allpad``: every position is ``padding_idx``; ``onepad``: random, one sample made of padding only."""
    g = gen(seed)
    M = (torch.randn(V, N, T, D, generator=g) * 10.0 ** (torch.rand(V, N, T, D, generator=g) * 2 - 1)).float()
    if pattern == "equal":
        idx = torch.full((N, T), W - 1, dtype=torch.int64)
    elif pattern == "distinct":
        assert W >= N * T
        idx = torch.randperm(W, generator=g)[:N * T].view(N, T)
    elif pattern == "allpad":
        idx = torch.full((N, T), padding_idx, dtype=torch.int64)
    else:
        idx = torch.randint(0, W, (N, T), generator=g)
        if pattern == "onepad":
            idx[N // 2] = padding_idx
    return Case(M, idx, W, padding_idx)
