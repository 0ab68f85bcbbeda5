"""Inputs off unit scale, degenerate inputs and ONE checker for the symmetric eigensolver (no GPU needed).

Every route of the solver carries LAPACK-style conditional scaling: outside the window 2^-20 <= amax <= 2^51 (amax = max
|a_ij|) the matrix is multiplied by a power of two sigma that brings amax to about one, and every route has its own place
where sigma is undone.  The inputs here move amax across both edges of that window, through its lower half (where 1/N-
normalised Gram matrices live and the solver runs unscaled), across the lower edge 2^-51 of LAPACK's ssyev and far outside;
the checker states the suite's bounds relative to ||A||_2 of the matrix AS GIVEN.

Rungs.  A rung k names log2(amax) after scaling, rounded AWAY from zero: k < 0 means 2^k <= amax < 2^(k+1), k > 0 means
2^(k-1) < amax <= 2^k, so that -20 and +51 lie just inside the solver's window and -21 and +52 just outside (and -51 / -52 likewise for
ssyev's lower edge), whatever the mantissa of amax.  Rung 0 is the matrix of ``make_matrix`` unchanged.  The shift is a
power of two applied in fp32."""
import functools
import hashlib

import numpy as np
import torch

from test_symeig_large_gpu import make_matrix, tridiag_case

KINDS = ("dense", "lowrank", "decay", "clustered")
RUNGS = (-120, -52, -51, -50, -21, -20, -10, 0, 50, 51, 52, 100)
SSYEV_RUNGS = (-51, -50, -21, -20, -10, 0, 50, 51)   # inside ssyev's window 2^-51 <= amax <= 2^51 (rung 0: amax ~ n)
UNSCALED_RUNGS = (-20, -10, 0, 50, 51)       # inside the solver's window: sigma = 1
RMIN, RMAX = 2.0 ** -20, 2.0 ** 51           # the solver's window (csrc/sytrd.hip:trd_sigma_kernel, csrc/symeig_small.hip)
FLT_MIN_NORMAL, FLT_DENORM = 2.0 ** -126, 2.0 ** -149
DENORMAL_LOG2_AMAX, NORM126_LOG2 = -130, 126
DEGENERATE = ("zero", "identity3", "diag_desc", "tridiag_wilkinson", "blockdiag", "dead_sample", "rank1", "neg_lowrank",
              "antidiag", "arrowhead")
SMALL_N_MAX = 192


def ulp32(x):
    """Spacing of fp32 at |x| (normal range)."""
    return float(np.spacing(np.float32(abs(x))))


def shift_to_rung(amax, rung):
    """log2 of the power of two that moves ``amax`` onto ``rung`` (see the module docstring)."""
    if rung == 0:
        return 0
    m, e = np.frexp(float(amax))                      # amax = m 2^e, 1/2 <= m < 1: floor(log2) = e - 1
    away = e - 1 if (rung < 0 or m == 0.5) else e     # log2(amax) rounded away from zero, for the sign of the rung
    return int(rung - away)


def ldexp32(A32, log2s):
    """``A32 * 2^log2s`` rounded once to fp32 (exact while nothing leaves the normal range)."""
    return torch.from_numpy(np.ldexp(A32.numpy(), np.int32(log2s)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _base(kind, n, seed):
    return make_matrix(kind, n, seed)


def scaled(kind, n, log2s, seed=0):
    """The fp32 matrix of ``make_matrix(kind, n, seed)`` (built in fp64, rounded to fp32) times 2^log2s in fp32."""
    return ldexp32(_base(kind, n, seed), log2s)


def on_rung(kind, n, rung, seed=0):
    """``scaled`` with the shift that puts amax on ``rung``; returns ``(A32, log2s)``."""
    log2s = shift_to_rung(float(_base(kind, n, seed).abs().max()), rung)
    return scaled(kind, n, log2s, seed), log2s


def norm126(n, seed=0):
    """``dense`` normalised in fp64 to ||A||_2 = 2^126, then rounded to fp32: no eigenvalue overflows."""
    g = torch.Generator().manual_seed(seed + n)
    M = torch.randn(n, n, generator=g, dtype=torch.float64)
    S = (M + M.T) / 2
    S = S * (2.0 ** NORM126_LOG2 / float(torch.linalg.eigvalsh(S).abs().max()))
    return ((S + S.T) / 2).float()


def denormal(kind, n, seed=0):
    """Every entry denormal: 2^-130 <= amax < 2^-129 (entries are multiples of 2^-149: 19 bits at most)."""
    A = _base(kind, n, seed)
    m, e = np.frexp(float(A.abs().max()))
    return scaled(kind, n, DENORMAL_LOG2_AMAX - (e - 1), seed)


def scaled_case(kind, n, rung, seed=0):
    """One input of the ladder by name: an integer rung, ``"norm126"`` or ``"denormal"``."""
    if rung == "norm126":
        return norm126(n, seed)
    if rung == "denormal":
        return denormal(kind, n, seed)
    return on_rung(kind, n, int(rung), seed)[0]


def scaled_tridiag(kind, n, rung, seed=0):
    """``tridiag_case`` of test_symeig_large_gpu.py with max(|d|, |e|) moved onto ``rung`` (exact)."""
    d, e = tridiag_case(kind, n, seed)
    amax = max(np.abs(d).max(), np.abs(e).max() if n > 1 else 0.0)
    s = np.int32(shift_to_rung(amax, rung))
    return np.ldexp(d, s).astype(np.float32), np.ldexp(e, s).astype(np.float32)


def degenerate(kind, n, log2s=0):
    """The degenerate inputs (fp32), times 2^log2s exactly."""
    f64 = torch.float64
    if kind == "zero":
        A = torch.zeros(n, n, dtype=f64)
    elif kind == "identity3":
        A = 3.0 * torch.eye(n, dtype=f64)
    elif kind == "diag_desc":      # distinct, descending: already diagonal, every reflector degenerate, order reversed
        A = torch.diag(torch.arange(n, 0, -1, dtype=f64))
    elif kind == "tridiag_wilkinson":   # W+ in dense storage: already tridiagonal, pairs of eigenvalues agreeing to fp32
        d = (torch.arange(n, dtype=f64) - n // 2).abs()
        A = torch.diag(d) + torch.diag(torch.ones(n - 1, dtype=f64), 1) + torch.diag(torch.ones(n - 1, dtype=f64), -1)
    elif kind == "blockdiag":      # e exactly 0 at the split after row n // 3
        k = n // 3
        A = torch.zeros(n, n, dtype=f64)
        A[:k, :k] = make_matrix("dense", k, 1).double()
        A[k:, k:] = make_matrix("dense", n - k, 2).double()
    elif kind == "dead_sample":    # a sample whose factor row is zero
        A = make_matrix("lowrank", n).double()
        A[n // 2, :] = 0.0
        A[:, n // 2] = 0.0
    elif kind == "rank1":
        u = torch.randn(n, generator=torch.Generator().manual_seed(7 + n), dtype=f64)
        A = torch.outer(u, u)
    elif kind == "neg_lowrank":
        A = -make_matrix("lowrank", n).double()
    elif kind == "antidiag":       # eigenvalues +1 (ceil(n/2) times) and -1 (floor(n/2) times)
        A = torch.flip(torch.eye(n, dtype=f64), [1])
    elif kind == "arrowhead":
        A = torch.diag(torch.arange(n, dtype=f64) / 4.0)
        A[0, 1:] = 1.0
        A[1:, 0] = 1.0
    else:
        raise ValueError(kind)
    A32 = ((A + A.T) / 2).float()
    return ldexp32(A32, log2s) if log2s else A32


# ---- the checker ----------------------------------------------------------------------------------------------------------
_REF = {}


def reference(A32):
    """``numpy.linalg.eigh`` of the fp32 matrix in fp64, computed once per distinct matrix."""
    a = np.ascontiguousarray(A32.numpy() if isinstance(A32, torch.Tensor) else A32, dtype=np.float32)
    key = (a.shape, hashlib.sha1(a.tobytes()).hexdigest())
    if key not in _REF:
        A64 = a.astype(np.float64)
        w, Z = np.linalg.eigh(A64)
        _REF[key] = (A64, w, Z)
    return _REF[key]


def _f64(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.float64)


def check_eigen(A32, w, Z=None, rows=None, *, small):
    """Eigenvalues ``w`` (all n, ascending) and, optionally, column eigenvectors ``Z`` [n, K] of the fp32 matrix ``A32``
    against fp64 LAPACK.  ``rows``: the indices into the ascending spectrum that the K columns of ``Z`` belong to (default:
    all n in order) -- a row range of ``symeig_rows`` or the selection of ``select``.  ``small``: the single-workgroup
    solver's bounds (n <= 192) instead of the multi-kernel solver's.

    Bounds, relative to ||A||_2 of the matrix as given:
      n > 192   eigenvalues 1e-5, orthonormality 5e-5, residual 3e-5   (test_symeig_large, test_two_stage_eigenvectors)
      n <= 192  eigenvalues 2e-5, orthonormality 2e-5, residual 5e-5   (test_symeig_small)
    A matrix whose entries are all denormal gets n 2^-149 added to the eigenvalue and residual bounds (the spacing of the
    input itself).  c I, c = 0 included: eigenvalues exact and Z^T Z - I below 1e-6 (test_two_stage_default_size_degenerate_
    inputs).  Any other diagonal matrix: eigenvalues equal the sorted diagonal to 1 ulp of ||A||_2.
    Prints the figures, then asserts; returns them."""
    A64, ref_w, _ = reference(A32)
    n = A64.shape[0]
    assert small == (n <= SMALL_N_MAX)
    tol_w, tol_orth, tol_res = (2e-5, 2e-5, 5e-5) if small else (1e-5, 5e-5, 3e-5)
    norm2 = float(np.abs(ref_w).max())
    amax = float(np.abs(A64).max())
    absolute = n * FLT_DENORM if 0.0 < amax < FLT_MIN_NORMAL else 0.0
    w = _f64(w)
    assert w.shape == (n,)
    assert np.isfinite(w).all(), "non-finite eigenvalue"
    diag = np.diag(A64)
    is_diag = not np.any(A64 - np.diag(diag))
    is_scalar = is_diag and bool(np.all(diag == diag[0]))
    fig = {"norm2": norm2, "eig": float(np.abs(w - ref_w).max())}
    rel = (lambda x: x / norm2) if norm2 > 0 else (lambda x: x)
    if Z is not None:
        Zc = _f64(Z)
        idx = np.arange(n) if rows is None else np.asarray(list(rows), dtype=np.int64)
        assert Zc.shape == (n, len(idx)), (Zc.shape, n, len(idx))
        assert np.isfinite(Zc).all(), "non-finite eigenvector entry"
        fig["orth"] = float(np.abs(Zc.T @ Zc - np.eye(len(idx))).max()) if len(idx) else 0.0
        fig["resid"] = float(np.abs(A64 @ Zc - Zc * w[idx][None, :]).max()) if len(idx) else 0.0
    print("check_eigen n=%d amax=2^%.2f: " % (n, np.log2(amax) if amax > 0 else -np.inf)
          + " ".join(f"{k}={rel(v) if k in ('eig', 'resid') else v:.3e}" for k, v in fig.items() if k != "norm2"))
    assert np.all(np.diff(w) >= 0), "eigenvalues not ascending"
    assert fig["eig"] <= tol_w * norm2 + absolute, ("eigenvalues", rel(fig["eig"]))
    if is_scalar:
        assert np.all(w == diag[0]), ("c I: eigenvalues not exact", float(np.abs(w - diag[0]).max()))
    elif is_diag:
        assert np.abs(w - np.sort(diag)).max() <= ulp32(norm2), ("diagonal", float(np.abs(w - np.sort(diag)).max() / ulp32(norm2)))
    if Z is not None:
        assert fig["orth"] < (1e-6 if is_scalar else tol_orth), ("orthonormality", fig["orth"])
        assert fig["resid"] <= tol_res * norm2 + absolute, ("residual", rel(fig["resid"]))
    return fig
