"""fp64 references and derived error bounds for the five kernels of the Embedding rule (csrc/embedding.hip).  TEST INFRASTRUCTURE
shared by tests/test_embedding_kernels_gpu.py and tests/test_embedding_refs_host.py; in the manner of tests/attention_refs.py.

Notation of include/vivit_hip.h: ``idx [N, T]`` token ids, ``M [V, N, T, D]`` the factor at the module output, ``W`` the vocabulary,
``Vt[v, n, w, :] = sum_{t: idx[n, t] = w} M[v, n, t, :]`` the weight factor (positions with ``idx == padding_idx`` contribute nothing).
The references are restated from ``M`` and ``idx`` in torch fp64 and never form a tensor with an axis of length ``W``: the tokens
that occur are renumbered ``0 .. Wr - 1`` first (``Wr <= N T``), which changes no sum.

Error bounds (u = 2^-24, elementwise against the fp64 reference; derived, not fitted).  An output that sums k products and additions
of fp32 numbers in ANY order, fused or not, has the error gamma_k sum|terms| at most, gamma_k = k u / (1 - k u) (Higham, Accuracy and
Stability of Numerical Algorithms, section 3.1: every term passes through at most k roundings).  sum|terms| is the same formula
evaluated on absolute values in fp64; k per output:

* compact  B[v, n, u, :]: the m rows of the slot are added, k = m (one row: a copy, and gamma_1 |x| >= 0 still holds).  The sum
           itself takes m - 1 roundings, so correct fp32 arithmetic can use up to (m - 1) / m of this bound and no more (gamma_{m-1} /
           gamma_m < (m - 1) / m): with T = 5 and repeated tokens a plain fp32 sum measures 0.57 of it (tests/test_embedding_refs_host.py).
           That is the one spare rounding of k = m, not slack to be tuned away.
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

from epilogue_refs import EPS, F64, gen, misaligned, within   # noqa: F401  (re-exported for the test modules)

SAMPLE_BLOCK = 16     # samples per sample block (EMB_SB of csrc/embedding.hip)
CLASS_CHUNK = 4       # classes per chunk (EMB_VC)
JOIN_PASS = 256       # entries of a sample block's token table the Gram kernel joins at a time
I32_MAX = 2 ** 31 - 1


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

    def block_tables(self):
        """Per block of 16 samples the sorted union of its (non-padding) tokens: the token table the Gram kernel joins."""
        out = []
        for n0 in range(0, self.N, SAMPLE_BLOCK):
            toks = self.idx[n0:n0 + SAMPLE_BLOCK].reshape(-1)
            out.append(torch.unique(toks if self.padding_idx is None else toks[toks != self.padding_idx]))
        return out

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


PATTERNS = ("equal", "distinct", "random", "allpad", "onepad", "staircase")


def make_case(seed, V, N, T, D, W, pattern="random", padding_idx=None, stride=None, base=0):
    """Seeded operands.  ``equal``: one token everywhere; ``distinct``: no token twice in the batch (needs W >= N T); ``random``: with
    repeats; ``allpad``: every position is ``padding_idx``; ``onepad``: random, one sample made of padding only; ``staircase``:
    sample n holds the tokens ``base + stride n + (0 .. T - 1)``, shuffled within the sample (``stride < T``; ``W`` is ignored and
    set to the largest token + 1)."""
    g = gen(seed)
    M = (torch.randn(V, N, T, D, generator=g) * 10.0 ** (torch.rand(V, N, T, D, generator=g) * 2 - 1)).float()
    if pattern == "equal":
        idx = torch.full((N, T), W - 1, dtype=torch.int64)
    elif pattern == "distinct":
        assert W >= N * T
        idx = torch.randperm(W, generator=g)[:N * T].view(N, T)
    elif pattern == "allpad":
        idx = torch.full((N, T), padding_idx, dtype=torch.int64)
    elif pattern == "staircase":
        assert 0 < stride < T
        idx = torch.stack([base + stride * n + torch.randperm(T, generator=g) for n in range(N)])
        W = base + stride * (N - 1) + T
    else:
        idx = torch.randint(0, W, (N, T), generator=g)
        if pattern == "onepad":
            idx[N // 2] = padding_idx
    return Case(M, idx, W, padding_idx)


# ---- the cases of tests/test_embedding_kernels_gpu.py (shared with tests/test_embedding_refs_host.py) -------------------------
# (T, D, V, N, W, pattern, padding_idx): a pruned product of T in {1, 2, 5, 17}, D in {1, 3, 4, 20, 64, 67}, V in {1, 3},
# N in {1, 2, 17, 33} (17 and 33 cross one and two sample-block edges), W in {1, 2, 7, 50} and the first five token patterns; then
# V in {4, 5, 8, 9} (class chunks: one full, two with one active wave in the second, two full, three) against N in {2, 17, 33}, the
# patterns random, onepad and equal, and D in {4, 20, 128, 129} (128: two full groups of four 16-column steps, 129: and a remainder)
CASES = [(1, 1, 1, 1, 1, "equal", None), (1, 3, 3, 2, 2, "random", None), (1, 4, 1, 17, 7, "random", 0), (1, 64, 3, 33, 50, "distinct", None),
         (2, 1, 3, 17, 50, "distinct", None), (2, 20, 1, 33, 7, "random", None), (2, 67, 3, 2, 2, "equal", None), (2, 4, 3, 2, 7, "onepad", 0),
         (5, 3, 1, 1, 1, "equal", None), (5, 4, 3, 17, 7, "random", 0), (5, 20, 3, 2, 50, "distinct", None), (5, 64, 1, 33, 50, "onepad", 0),
         (5, 67, 3, 33, 7, "random", None), (5, 20, 3, 17, 7, "allpad", 0),
         (17, 1, 3, 2, 7, "random", None), (17, 3, 3, 17, 50, "random", 3), (17, 20, 1, 2, 1, "equal", None), (17, 64, 3, 17, 2, "random", None),
         (17, 67, 1, 33, 50, "random", 0), (17, 4, 3, 33, 50, "allpad", 0), (17, 20, 3, 33, 50, "onepad", 5), (17, 64, 3, 33, 7, "equal", None),
         (5, 20, 5, 17, 7, "random", 0), (2, 4, 8, 33, 50, "random", None), (17, 129, 9, 2, 2, "equal", None), (5, 128, 4, 17, 7, "onepad", 0),
         (17, 3, 5, 33, 50, "random", 3), (5, 129, 5, 33, 7, "onepad", 0), (2, 20, 9, 17, 7, "equal", None), (5, 4, 9, 33, 50, "random", None),
         (17, 128, 8, 2, 50, "random", 5), (1, 20, 4, 33, 2, "equal", None), (5, 20, 8, 2, 7, "onepad", 0), (2, 129, 4, 17, 50, "random", None)]


def case_of(T, D, V, N, W, pattern, pad):
    return make_case(100000 * T + 1000 * D + 10 * N + V, V, N, T, D, W, pattern, pad)


# Staircase constructions (N, T, S): consecutive samples share T - S tokens, the table of a full sample block is the run of its
# 15 S + T tokens, so the rank of a token in its block's table is its offset from the block's first token.  ``table``: the length of
# block 0's table; ``shared``: (n, m, the ranks of the tokens n and m share in n's block, the same in m's block).
#   (17, 17, 16)  257 entries: the second pass of the join holds one, token 256, which sample 16 (the next sample block) shares
#   (33, 20, 17)  275 entries: samples 14 and 15 share the ranks 255, 256, 257, on both sides of the pass edge; samples 15 and 16
#                 share the ranks 272 .. 274 of block 0 = 0 .. 2 of block 1, found by the block pair (1, 0) in the 275-entry table
#   (16, 31, 15)  256 entries: exactly one pass
STAIRCASE = {(17, 17, 16): dict(table=257, shared=[(15, 16, [256], [0])]),
             (33, 20, 17): dict(table=275, shared=[(14, 15, [255, 256, 257], [255, 256, 257]), (15, 16, [272, 273, 274], [0, 1, 2])]),
             (16, 31, 15): dict(table=256, shared=[(14, 15, list(range(225, 241)), list(range(225, 241)))])}
STAIRCASE_CASES = [(N, T, S, V, D) for (N, T, S) in STAIRCASE for V in (5, 9) for D in (4, 20)]


def staircase_of(N, T, S, V, D):
    return make_case(10000 * N + 100 * S + 10 * V + D, V, N, T, D, None, "staircase", stride=S)


def check_staircase(case, N, T, S):
    """The construction does what the list says it does, from the ``Case`` alone."""
    want = STAIRCASE[(N, T, S)]
    tabs = case.block_tables()
    assert tabs[0].numel() == want["table"] == (SAMPLE_BLOCK - 1) * S + T
    assert (tabs[0].numel() > JOIN_PASS) == (want["table"] > JOIN_PASS)
    for n, m, ranks_n, ranks_m in want["shared"]:
        common = torch.tensor(sorted(set(case.idx[n].tolist()) & set(case.idx[m].tolist())))
        assert common.numel() == T - S == len(ranks_n)
        for s, ranks in ((n, ranks_n), (m, ranks_m)):
            tab = tabs[s // SAMPLE_BLOCK]
            at = torch.searchsorted(tab, common)
            assert torch.equal(tab[at], common) and at.tolist() == ranks, (n, m, at.tolist())


# tokens up to 2^31 - 2, the largest an int32 id below num_embeddings = 2^31 - 1 can be; once with the smallest of them as padding
LARGE_BASE = I32_MAX - 1 - (3 * 1 + 4)


def large_id_case(pad):
    case = make_case(77, 4, 2, 5, 129, None, "staircase", LARGE_BASE if pad else None, stride=3, base=LARGE_BASE)
    assert int(case.idx.max()) == I32_MAX - 1 and case.W == I32_MAX and int((case.idx == LARGE_BASE).sum()) == 1
    return case
