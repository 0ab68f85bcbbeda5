"""Child process of tests/test_gemm_output_gpu.py: the OUTPUT side and the workspace of every route of the public products
(vivit_gemm_{nt,nn,tn}_f32, vivit_gram_syrk_f32) through the raw C ABI, in the environment it was started with (the route
switches are read once per process).

    python gemm_output_child.py MODE out.json digests.json        MODE: a key of MODES, started with its environment

out.json: {case: "ok" | text with every failed check of the case}; digests.json: {name: sha256 of an output} for the
comparisons between the two processes.  Inputs are the seeded N(0, 1) operands of gemm_contract_child.operands.

Every case of cases(mode) runs, per (alpha, beta) in SETTINGS ((1, 0) over an `out` left NaN, (0.5, -2) and (1, 1) over a seeded C0):
  1. the entry point on a helpers.Guarded workspace of EXACTLY the bytes its query asks for and a contiguous `out`: status OK,
     the pattern on both sides of the workspace intact, `out` byte-equal to the vivit_amd.kernels wrapper's (which allocates
     1.25 x the query + 256 bytes);
  2. the same with `out` a window [M, N] at row 1, column 1 of NaN-filled storage [M + 2, N + 7] (ldc = N + 7 is odd and C is
     4 bytes off a 16-byte boundary): every element outside the window still has the NaN's bits, the window is byte-equal to
     the contiguous `out` (ldc changes addresses, not the order of any sum: gemm_launch chooses its route from the alignment
     of A and B, not of C); a SYRK window is exactly symmetric and, for p >= 1024, its diagonal is the fp64 value of
     alpha sum_k a_ik^2 + beta C0_ii rounded once to fp32 (syrk_diag_kernel) -- on every workspace that has room for its n
     floats, shorter than the query or not; without that room the diagonal must be within bound 3;
  3. every entry within   5e-6 |alpha| ||a_i|| ||b_j|| + (L + 2) 2^-24 (|beta C0_ij| + |alpha| ||a_i|| ||b_j||)   of
     alpha a b^T + beta C0 in fp64 on the device.  First term: the project's bound (test_gemm_contract_gpu.py); second: the
     roundings of the beta path -- one for beta * C, one per launch that adds into C (L: the chunks of 4096 columns of
     Tile256Bx plus the ragged K tail; 1 on every other route, whose partial sums meet in a slab or in registers), one for
     the final add.
short_cases(mode) run on workspaces SHORTER than the query (the last column of the route table in csrc/gemm_plan.h); the
other functions: K == 0, the NULL workspace of the 256 tile, and (split0) the re-plan of Tile256 to the splits a workspace
holds.
"""
import hashlib
import json
import sys

import torch

from helpers import Guarded  # (importing helpers puts the repository root on sys.path)
import gemm_contract_child as contract
from vivit_amd import _lib, kernels

DEV = contract.DEV
SETTINGS = ((1.0, 0.0), (0.5, -2.0), (1.0, 1.0))
EPS = 2.0 ** -24
LIB = _lib.load()
MODES = {"default": {}, "split0": {"VIVIT_GEMM_SPLIT": "0"}}   # the environment of each child process


# (name, layout, M, N, K, leading dimensions of K-contiguous operands rounded up to this many floats, L of the bound).
# Each shape is the smallest that still reaches its route (the predicate named) with ragged edge tiles.
def cases(mode):
    out = [
        # plan_tile256: 15 x 14 = 210 >= 200 tiles of 256 x 256, both edges ragged, M, N % 4 == 0 (NN / TN operands stay 16-byte
        # aligned); K = 6151: whole K tiles 6144 = two public chunks (4096 + 2048, bx_chunk_cols) + a ragged tail of 7 through
        # gemm_kernel, so L = 3 (split0: gemm256_kernel in one launch + the tail, L = 2)
        *[(f"tile256-{lay}", lay, 3588, 3400, 6151, 4, 3 if mode == "default" else 2) for lay in contract.LAYOUTS],
        # 20 tile rows = 210 lower tiles, lda = 6152: the mirror only on the last chunk, bx_sym_diag_kernel, the fp64 diagonal
        ("tile256-syrk", "syrk", 4868, 4868, 6151, 4, 3 if mode == "default" else 2),
    ]
    if mode == "default":
        out += [
            # plan_bx_splitk: M, N >= 256, 4 x 6 = 24 <= 100 tiles, K >= 16384, K % 16 == 0 (N, M % 4 == 0 for NN / TN)
            *[(f"splitk-{lay}", lay, 1000, 1300, 16384, 1, 1) for lay in contract.LAYOUTS],
            ("splitk-syrk", "syrk", 1280, 1280, 16384, 1, 1),   # 15 lower tiles
            # plan_gemm64: M <= 64, N >= 2048, K >= 2048, K % 16 == 0; NN: M > 16 (skinny_applicable takes M <= 16 first) and
            # N % 4 == 0; TN: M % 4 == 0
            *[(f"gemm64-{lay}", lay, 36, 2100, 2064, 1, 1) for lay in contract.LAYOUTS],
            ("gemm64-nt-1row", "nt", 1, 2048, 2048, 1, 1),
            # plan_tsk: M <= 64, N <= 1024 (so not Gemm64), K >= 2048, K % 4 == 0, NT only
            ("tsk-nt", "nt", 48, 700, 2048, 1, 1),
            # skinny_applicable: 1 <= M <= 16 (vivit_gemm_nn_f32 only).  skinny_nn_kernel tiles N by 1024 columns and K by chunks of
            # 1024 rows, 8 rows per trip, and is instantiated for 1, 2, 4, 8, 16 rows of the output.  Smaller than the issue's
            # 8 x 5000 x 3000: M = 3 (instance 4, one row idle), two column blocks, two row chunks, the second of 3 rows; N = 1028 keeps
            # the 16-byte loads and stores (one live lane in the last block), N = 1030 takes the scalar ones with their column guards
            ("skinny-nn-vec", "nn", 3, 1028, 1027, 1, 1),
            ("skinny-nn-scalar", "nn", 3, 1030, 1027, 1, 1),
            # gemm_kernel (plan_tile128).  300 x 300 x 1009: 9 tiles, 64 K tiles -> two splits and a slab; NT / NN: lda = 1009 is
            # not a multiple of 4; TN: too small for the streaming routes
            *[(f"generic-slab-{lay}", lay, 300, 300, 1009, 1, 1) for lay in contract.LAYOUTS],
            *[(f"generic-{lay}", lay, 130, 250, 37, 1, 1) for lay in contract.LAYOUTS],   # 3 K tiles: no slab
            ("generic-syrk", "syrk", 200, 200, 333, 1, 1),   # p < 1024: the product's own diagonal
        ]
    return out


def short_cases(mode):
    """Shorter workspaces: every non-SYRK nt case and the two SYRK cases of the 256 tile (Tile256Bx, BxSplitK)."""
    return [c for c in cases(mode) if c[1] == "nt" or c[0] in ("tile256-syrk", "splitk-syrk")]


# plan_tile256 for 4096 x 4352 x 8192 (16 x 17 = 272 tiles): one split fills 272 / 512 of two rounds (0.53 < 0.6: refused), two
# 0.68, three 0.75, four 0.78 -> four splits of 2048 k, a slab of 4 M N 4 = 285 MB
REPLAN = ("replan", "nt", 4096, 4352, 8192, 1, 1)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bytes(x, y):
    return x.shape == y.shape and torch.equal(bits(x), bits(y))


def digest(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


class Run:
    """One launch: status, the guarded workspace, the whole storage of C with its bits before the launch, and the [M, N] view."""

    def __init__(self, status, guard, storage, before, out, window):
        self.status, self.guard, self.storage, self.before, self.out, self.window = status, guard, storage, before, out, window

    def guard_intact(self, fails, what):
        try:
            self.guard.assert_intact()
        except AssertionError as e:
            fails.append(f"{what}: {e}")

    def padding_intact(self):
        """Every element of the storage outside the window still has the bits it had (NaN)."""
        now, was = self.storage.view(torch.int32).clone(), self.before.clone()
        m, n = self.out.shape
        now[1:m + 1, 1:n + 1] = 0
        was[1:m + 1, 1:n + 1] = 0
        return torch.equal(now, was)


class Problem:
    def __init__(self, name, lay, m, n, k, align, launches):
        self.name, self.lay, self.m, self.n, self.k, self.launches = name, lay, m, n, k, launches
        self.syrk = lay == "syrk"
        a, b = contract.operands((lay, m, n, k))
        self.a, self.b = a, (a if self.syrk else b)   # logical operands: the product is a b^T
        self.A = a.T.contiguous() if lay == "tn" else contract._padded(a, align)
        self.B = None if self.syrk else contract._padded(b, align) if lay == "nt" else b.T.contiguous()
        self._ref = None

    def c0(self):
        g = torch.Generator(device=DEV).manual_seed(self.m * 7919 + self.n * 31 + self.k)
        c = torch.randn(self.m, self.n, generator=g, device=DEV)
        return c + c.T if self.syrk else c   # (a SYRK computes the lower tiles and mirrors them)

    def query(self):
        if self.syrk:
            return LIB.vivit_gram_syrk_f32_workspace_bytes(self.n, self.k)
        return LIB.vivit_gemm_f32_workspace_bytes(self.m, self.n, self.k)

    def raw(self, C, ldc, alpha, beta, ws, ws_bytes):
        s = torch.cuda.current_stream().cuda_stream
        if self.syrk:
            return LIB.vivit_gram_syrk_f32(self.A.data_ptr(), self.n, self.k, kernels._ld(self.A), C.data_ptr(), ldc, alpha, beta, ws,
                                         ws_bytes, s)
        return getattr(LIB, f"vivit_gemm_{self.lay}_f32")(self.A.data_ptr(), self.B.data_ptr(), C.data_ptr(), self.m, self.n, self.k,
                                                       kernels._ld(self.A), kernels._ld(self.B), ldc, alpha, beta, ws, ws_bytes, s)

    def wrapper(self, out, alpha, beta):
        if self.syrk:
            return kernels.gram_syrk(self.A, out=out, alpha=alpha, beta=beta)
        return getattr(kernels, f"gemm_{self.lay}")(self.A, self.B, out=out, alpha=alpha, beta=beta)

    def run(self, alpha, beta, c0, window, ws_bytes=None):
        """The entry point on a guarded workspace of exactly `ws_bytes` (default: the query; 0: a NULL pointer).  `out` is NaN where
        `c0` is None; with `window` it sits at [1, 1] of NaN-filled storage [M + 2, N + 7]."""
        m, n = self.m, self.n
        storage = torch.full((m + 2, n + 7) if window else (m, n), float("nan"), device=DEV)
        out = storage[1:m + 1, 1:n + 1] if window else storage
        if c0 is not None:
            out.copy_(c0)
        before = storage.view(torch.int32).clone()
        guard = Guarded(self.query() if ws_bytes is None else ws_bytes)
        st = self.raw(out, n + 7 if window else n, alpha, beta, guard.ptrs[0], guard.sizes[0])
        torch.cuda.synchronize()
        return Run(st, guard, storage, before, out, window)

    def reference(self):
        if self._ref is None:
            ad, bd = self.a.double(), self.b.double()
            self._ref = (ad @ bd.T, ad.norm(dim=1)[:, None] * bd.norm(dim=1)[None, :])
        return self._ref

    def bound_failure(self, got, alpha, beta, c0, diagonal=False):
        """None, or how `got` (`diagonal`: its diagonal alone) misses bound 3 of the module docstring."""
        prod, scale = self.reference()
        if diagonal:
            got, prod, scale, c0 = got.diagonal()[None], prod.diagonal()[None], scale.diagonal()[None], None if c0 is None else c0.diagonal()[None]
        old = beta * c0.double() if (c0 is not None and beta != 0.0) else torch.zeros_like(prod)
        s = abs(alpha) * scale
        bound = 5e-6 * s + (self.launches + 2) * EPS * (old.abs() + s)
        err = (got.double() - (alpha * prod + old)).abs()
        bad = ~(err <= bound)   # (a NaN is bad)
        if not bad.any():
            return None
        i, j = (int(x) for x in bad.nonzero()[0])
        return f"{int(bad.sum())} {'diagonal ' if diagonal else ''}entries miss the fp64 bound, first at ({i}, {j}): error {err[i, j].item():.3e}, bound {bound[i, j].item():.3e}"

    def diagonal_failure(self, got, alpha, beta, c0):
        """None, or how the diagonal of a public SYRK with p >= 1024 differs from fp64 rounded once: |got - exact| <= ulp(got) / 2
        (+ 2^-40 relative for the order of the fp64 sum)."""
        exact = alpha * (self.a.double() ** 2).sum(1)
        if c0 is not None and beta != 0.0:
            exact = exact + beta * c0.diagonal().double()
        d = got.diagonal()
        half_ulp = torch.ldexp(torch.ones_like(exact), torch.frexp(d)[1] - 25)   # d = f 2^e, f in [0.5, 1): ulp = 2^(e - 24)
        bad = ~((d.double() - exact).abs() <= half_ulp + 2.0 ** -40 * exact.abs())
        if not bad.any():
            return None
        i = int(bad.nonzero()[0])
        return f"{int(bad.sum())} diagonal entries are not the fp64 value rounded once, first {i}: {d[i].item()!r} for {exact[i].item()!r}"


def check_window(prob, run, contiguous, alpha, beta, c0, fails, what):
    """Checks 2 and 3 on a successful window launch; `contiguous`: the same launch on a contiguous `out`."""
    run.guard_intact(fails, what)
    if not run.padding_intact():
        fails.append(f"{what}: storage outside the window was written")
    got = run.out.contiguous()
    # ldc changes addresses, not the order of any sum (no kernel of these routes was found to choose a summation order from C)
    equal = same_bytes(got, contiguous)
    if not equal:
        fails.append(f"{what}: window differs from the contiguous out ({int((bits(got) != bits(contiguous)).sum())} entries)")
    for name, c in (("window", got),) + (() if equal else (("contiguous out", contiguous),)):
        miss = prob.bound_failure(c, alpha, beta, c0)
        if miss:
            fails.append(f"{what}, {name}: {miss}")
    if prob.syrk:
        if not same_bytes(got, got.T):
            fails.append(f"{what}: SYRK window is not symmetric")
        # The fp64 diagonal (p >= 1024) needs n floats in FRONT of the GEMM's workspace: syrk_diag_bytes(n) = 4 n rounded up to
        # 256, + 256 bytes.  vivit_gram_syrk_f32 takes them from every workspace that has them and whose rest the product
        # accepts, so every successful launch here with that much workspace must have the correctly rounded diagonal.  Below
        # that (NULL; the VIVIT_GEMM_SPLIT=0 query, which is nothing but these bytes, cut short) the old diagonal has nowhere
        # to wait while the product overwrites it: the diagonal is the product's own and must be within bound 3.
        if prob.k >= 1024:
            room = run.guard.sizes[0] >= -(-4 * prob.n // 256) * 256 + 256
            miss = prob.diagonal_failure(got, alpha, beta, c0) if room else prob.bound_failure(got, alpha, beta, c0, diagonal=True)
            if miss:
                fails.append(f"{what}: {miss}")


def case_output(prob):
    fails, c0 = [], prob.c0()
    for alpha, beta in SETTINGS:
        what = f"alpha {alpha} beta {beta}"
        init = None if beta == 0.0 else c0
        exact = prob.run(alpha, beta, init, window=False)
        if exact.status != _lib.VIVIT_OK:
            fails.append(f"{what}: status {exact.status} on exactly the query ({exact.guard.sizes[0]} bytes)")
            continue
        exact.guard_intact(fails, f"{what}, contiguous out")
        want = prob.wrapper(c0.clone() if init is not None else torch.full_like(c0, float("nan")), alpha, beta)
        if not same_bytes(exact.out, want):
            fails.append(f"{what}: output on exactly the query differs from the wrapper's")
        win = prob.run(alpha, beta, init, window=True)
        if win.status != _lib.VIVIT_OK:
            fails.append(f"{what}: status {win.status} with a window as out")
            continue
        check_window(prob, win, exact.out, alpha, beta, init, fails, f"{what}, window")
    return fails


def case_short(prob, must_succeed):
    """Workspaces of 0 (NULL), half the query (rounded down to 256) and query - 1 bytes: OK with checks 2 and 3, or
    VIVIT_E_WORKSPACE with nothing written."""
    fails, c0, q = [], prob.c0(), prob.query()
    alpha, beta = 0.5, -2.0
    if must_succeed:
        # a 256-tile shape on less than its query runs gemm256_kernel in ONE launch plus the ragged K tail, whatever the process:
        # the bf16 pieces never fit (SYRK: not behind the diagonal's bytes either), so L = 2
        prob.launches = 2
    if q == 0:
        print(f"  {prob.name}: the query is 0 bytes: nothing to shorten, no launch made here", flush=True)
    for w in sorted({0, q // 2 // 256 * 256, q - 1}):
        if not 0 <= w < q:
            continue
        what = f"{w} of {q} bytes"
        win = prob.run(alpha, beta, c0, window=True, ws_bytes=w)
        print(f"  {prob.name}: {what}: status {win.status}", flush=True)
        if win.status == _lib.VIVIT_E_WORKSPACE and not must_succeed:
            win.guard_intact(fails, what)
            if not torch.equal(win.storage.view(torch.int32), win.before):
                fails.append(f"{what}: refused, but C was written")
        elif win.status == _lib.VIVIT_OK:
            flat = prob.run(alpha, beta, c0, window=False, ws_bytes=w)
            if flat.status != _lib.VIVIT_OK:
                fails.append(f"{what}: status {flat.status} with a contiguous out, OK with a window")
                continue
            flat.guard_intact(fails, f"{what}, contiguous out")
            check_window(prob, win, flat.out, alpha, beta, c0, fails, what)
        else:
            fails.append(f"{what}: status {win.status}")
    return fails


def case_empty():
    """K == 0: C = beta C without a product; beta = 0 does not read C."""
    fails = []
    prob = Problem("empty", "nt", 64, 64, 0, 1, 1)
    c0 = prob.c0()
    if prob.query() != 0:
        fails.append(f"the query asks for {prob.query()} bytes")
    for beta, init, want in ((0.0, None, torch.zeros_like(c0)), (-2.0, c0, -2.0 * c0)):
        win = prob.run(1.0, beta, init, window=True)
        if win.status != _lib.VIVIT_OK:
            fails.append(f"beta {beta}: status {win.status}")
            continue
        if not win.padding_intact():
            fails.append(f"beta {beta}: storage outside the window was written")
        if not same_bytes(win.out, want):
            fails.append(f"beta {beta}: window is not exactly beta * C0")
    return fails


def case_null_workspace(prob, mode, digests):
    """The 256 tile with a NULL workspace: OK, and NOT the bytes of the full-workspace product where that one runs the bf16 pipe
    (default); the digest goes to the parent, which compares the two processes (the same gemm256_kernel with one split)."""
    fails = []
    null = prob.run(1.0, 0.0, None, window=False, ws_bytes=0)
    if null.status != _lib.VIVIT_OK:
        return [f"status {null.status} with a NULL workspace"]
    miss = prob.bound_failure(null.out, 1.0, 0.0, None)
    if miss:
        fails.append(miss)
    digests[f"{prob.name}-null"] = digest(null.out)
    if mode == "default":
        full = prob.run(1.0, 0.0, None, window=False)
        if full.status != _lib.VIVIT_OK:
            fails.append(f"status {full.status} on the whole query")
        elif same_bytes(full.out, null.out):
            fails.append("a NULL workspace gave the bytes of the full-workspace product: no fall-back to the fp32 kernel happened")
    return fails


def case_replan():
    """gemm_launch re-plans Tile256 to the splits the workspace holds (fit = workspace_bytes / (M N 4)): the query (four splits),
    exactly two slabs (two) and four bytes less (one, which needs none).  Different split counts, different summation orders."""
    fails = []
    prob = Problem(*REPLAN)
    c0, q, slab = prob.c0(), prob.query(), prob.m * prob.n * 4
    if q < 2 * slab:
        return [f"the query ({q} bytes) is below two slabs ({2 * slab}): plan_tile256 no longer splits this shape"]
    outs = []
    for w in (q, 2 * slab, 2 * slab - 4):
        win = prob.run(0.5, -2.0, c0, window=True, ws_bytes=w)
        if win.status != _lib.VIVIT_OK:
            fails.append(f"{w} bytes: status {win.status}")
            continue
        win.guard_intact(fails, f"{w} bytes")
        if not win.padding_intact():
            fails.append(f"{w} bytes: storage outside the window was written")
        got = win.out.contiguous()
        miss = prob.bound_failure(got, 0.5, -2.0, c0)
        if miss:
            fails.append(f"{w} bytes: {miss}")
        for w2, other in outs:
            if same_bytes(got, other):
                fails.append(f"{w} and {w2} bytes gave the same bytes: the same number of splits")
        outs.append((w, got))
    return fails


def jobs(mode, digests=None):
    """(name, function) of everything the process of `mode` runs, in order."""
    out = [(f"output-{c[0]}", lambda c=c: case_output(Problem(*c))) for c in cases(mode)]
    out += [(f"short-{c[0]}", lambda c=c: case_short(Problem(*c), must_succeed=c[0].startswith("tile256"))) for c in short_cases(mode)]
    out += [("empty-contraction", case_empty)]
    out += [(f"null-{c[0]}", lambda c=c: case_null_workspace(Problem(*c), mode, digests)) for c in cases(mode)
            if c[0] in ("tile256-nt", "tile256-syrk")]
    if mode == "split0":
        out += [("replan-tile256", case_replan)]
    return out


def main(mode, out_path, digest_path):
    assert (LIB.vivit_gemm_split_mode() == 0) == (mode == "split0"), "the mode and VIVIT_GEMM_SPLIT disagree"
    res, digests = {}, {}
    for name, fn in jobs(mode, digests):
        try:
            fails = fn()
            res[name] = "ok" if not fails else "; ".join(fails)
        except AssertionError as e:
            res[name] = f"AssertionError: {e}"
        except RuntimeError as e:
            res[name] = f"RuntimeError: {e}"
            break   # possibly a device error: nothing more runs on the GPU in this process
        finally:
            print(name, res.get(name), flush=True)
            with open(out_path, "w") as f:
                json.dump(res, f)
            with open(digest_path, "w") as f:
                json.dump(digests, f)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], sys.argv[3])
