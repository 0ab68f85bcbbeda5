"""Every route of the symmetric eigensolver off unit scale.

Each route carries its own copy of the LAPACK-style conditional scaling (a power of two sigma that brings amax to about
one outside 2^-20 .. 2^51) and its own place where sigma is undone; at the scales of the rest of the suite sigma is exactly 1.
Here the inputs of tests/eig_edge_refs.py walk amax far below the window, across the lower edge of LAPACK's ssyev (2^-51),
across the solver's own lower edge (2^-21, 2^-20), through the lower half of the window (2^-10: the solver runs unscaled on
Householder squares, rotations and a deflation tolerance that must follow ||T||), across the upper edge, far above, to
||A||_2 = 2^126 and to a fully denormal matrix -- through each route at the smallest size that reaches it.  ``check_eigen``
holds every result to the suite's bounds relative to ||A||_2 of the matrix as given; tests/test_eig_edge_refs_host.py shows
that fp64 LAPACK rounded to fp32 meets them all.  One test case runs one (route, kind, size) over the whole ladder and names
every rung that fails.

Routes chosen by ``VIVIT_TWO_STAGE`` (read once per process) run in ONE child process for all their cases."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import eig_edge_refs as R
import symeig_scale_child as C
from vivit_amd import kernels

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
HERE = os.path.dirname(os.path.abspath(__file__))
GGN_KINDS = ("lowrank", "decay")
LADDER = list(R.RUNGS) + ["denormal"]

# (route, sizes, kinds) in this process; the reduction is the default one of the size
IN_PROCESS = [
    ("full", (2, 33, 192), GGN_KINDS),            # single workgroup
    ("full", (200, 516), R.KINDS),                # persistent one-stage
    ("chain", (200,), R.KINDS),                   # launch-chain one-stage
    ("rows", (200,), GGN_KINDS),
    ("band", (200,), GGN_KINDS),
    ("select", (200,), GGN_KINDS),
    ("select_dc", (516,), GGN_KINDS),
]
TWO_STAGE = [("full", (200,), R.KINDS), ("rows", (200,), GGN_KINDS), ("select", (200,), GGN_KINDS)]
BATCH_RUNGS = [(-100, 0, 100), (-51, -52, 52), (-120, 51, "denormal"), (-21, -20, -10)]
EQUIVARIANCE = [("full", 192), ("full", 200), ("chain", 200), ("rows", 200), ("band", 200), ("select", 200)]
EQUIVARIANCE_RUNGS = (-50, -20, -10, 50)


def expand(table):
    """(route, kind, n, ladder): ``dense`` also takes the ||A||_2 = 2^126 case (on routes without ``dense``: that case alone)."""
    out = []
    for route, sizes, kinds in table:
        for n in sizes:
            out += [(route, kind, n, tuple(LADDER) + (("norm126",) if kind == "dense" else ())) for kind in kinds]
            if "dense" not in kinds:
                out.append((route, "dense", n, ("norm126",)))
    return out


def case_id(c):
    return "-".join(str(x) for x in c[:3]) if isinstance(c[-1], tuple) and len(c) == 4 else "-".join(str(x) for x in c)


@pytest.mark.parametrize("route,kind,n,rungs", expand(IN_PROCESS), ids=[case_id(c) for c in expand(IN_PROCESS)])
def test_scaled_input(route, kind, n, rungs):
    C.check_all(route, [(f"rung {rung}", [R.scaled_case(kind, n, rung)], None) for rung in rungs])


@pytest.mark.parametrize("kind", GGN_KINDS)
@pytest.mark.parametrize("route,n", [("batched_values", 64), ("batched_values", 200), ("batched_select", 200)])
def test_batch_of_mixed_scales(route, n, kind):
    """Three problems of one launch on three different rungs: each is checked like a single solve and is byte-identical to
    its single solve at the same scale (a per-problem sigma read from another problem's slot breaks both)."""
    C.check_all(route, [(f"rungs {rungs}", [R.scaled_case(kind, n, rung, seed=i) for i, rung in enumerate(rungs)], None)
                        for rungs in BATCH_RUNGS])


def assert_equivariant(figs):
    bad = {rung: fig for rung, fig in figs.items() if not (fig["eig_ulps"] <= 2.0 and fig["vec"] <= 1e-5)}
    assert not bad, bad


@pytest.mark.parametrize("route,n", EQUIVARIANCE, ids=[case_id(c) for c in EQUIVARIANCE])
def test_scale_equivariance(route, n):
    """symeig(2^k A) against 2^k symeig(A), A on rung 0, on rungs where sigma is 1 (-20, -10, 50) or an exact power of two
    (-50): eigenvalues within 2 ulp of ||A||_2, eigenvectors within 1e-5 after sign alignment.  Not bit equality: nothing
    promises it."""
    assert_equivariant({rung: C.equivariance(route, n, rung) for rung in EQUIVARIANCE_RUNGS})


@pytest.mark.parametrize("n", [33, 200])
def test_entry_above_3e38_is_rejected(n):
    """The header's statement for input the scan calls non-finite: info = n, which the launcher raises as RuntimeError."""
    A = R.scaled("dense", n, 0).clone()
    A[n // 2, 1] = A[1, n // 2] = 3.2e38
    infos = []
    kernels.symeig(A.to(C.DEV), eigenvectors=True, info_out=infos)
    assert int(infos[0].item()) == n
    with pytest.raises(RuntimeError):
        kernels.symeig(A.to(C.DEV), eigenvectors=False)


@pytest.mark.parametrize("n", [33, 200])
def test_eigenvalue_beyond_flt_max_comes_back_as_inf(n):
    """What the header states for a finite matrix whose largest eigenvalue (n 2^126) is no fp32 number: +inf with info = 0,
    every other eigenvalue and the eigenvectors finite."""
    A = torch.full((n, n), 2.0 ** 126, device=C.DEV)
    for vec in (False, True):
        infos = []
        w, Z = kernels.symeig(A, eigenvectors=vec, info_out=infos)
        assert int(infos[0].item()) == 0
        assert float(w[-1]) == float("inf") and bool(w[:-1].isfinite().all())
        assert Z is None or bool(Z.isfinite().all())


# ---- the two-stage reduction at n = 200: one child for all its cases ----------------------------------------------------------
def run_child(tmp, tag, cases, **env):
    cases_path, out = tmp / f"{tag}_cases.json", tmp / f"{tag}_out.json"
    cases_path.write_text(json.dumps(cases))
    proc = subprocess.run([sys.executable, os.path.join(HERE, "symeig_scale_child.py"), str(cases_path), str(out)],
                          env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-2000:]
    return json.loads(out.read_text())


TWO_STAGE_GROUPS = expand(TWO_STAGE)
TWO_STAGE_CASES = [{"id": case_id(c[:3] + (rung,)), "fn": "route", "route": c[0], "inputs": [["scaled", c[1], c[2], rung]]}
                   for c in TWO_STAGE_GROUPS for rung in c[3]]
TWO_STAGE_EQUIV = [{"id": f"equivariance-{route}-{rung}", "fn": "equivariance", "route": route,
                    "inputs": [["scaled", "dense", 200, rung]]} for route in ("full", "rows", "select")
                   for rung in EQUIVARIANCE_RUNGS]


@pytest.fixture(scope="module")
def two_stage(tmp_path_factory):
    return run_child(tmp_path_factory.mktemp("scale"), "two_stage", TWO_STAGE_CASES + TWO_STAGE_EQUIV, VIVIT_TWO_STAGE="1")


def assert_child_cases(results, ids):
    missing = [i for i in ids if i not in results]
    assert not missing, f"the child stopped before {missing}"
    failed = [f"{i}: {results[i]['err']}" for i in ids if not results[i]["ok"]]
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("route,kind,n,rungs", TWO_STAGE_GROUPS, ids=[case_id(c) for c in TWO_STAGE_GROUPS])
def test_scaled_input_two_stage(two_stage, route, kind, n, rungs):
    assert_child_cases(two_stage, [case_id((route, kind, n, rung)) for rung in rungs])


@pytest.mark.parametrize("route", ["full", "rows", "select"])
def test_scale_equivariance_two_stage(two_stage, route):
    ids = {rung: f"equivariance-{route}-{rung}" for rung in EQUIVARIANCE_RUNGS}
    assert_child_cases(two_stage, list(ids.values()))
    assert_equivariant({rung: two_stage[i]["fig"] for rung, i in ids.items()})


# ---- the tridiagonal solver alone, at the edges of the range the full solver guarantees to it -------------------------------
@pytest.mark.parametrize("rung", [-50, 50])
@pytest.mark.parametrize("n", [65, 500])
@pytest.mark.parametrize("kind", ["random", "wilkinson", "clustered", "decoupled", "graded"])
def test_stedc_at_the_window_edges(kind, n, rung):
    """The cases and bounds of test_symeig_large_gpu.py::test_stedc with max(|d|, |e|) on 2^-50 and 2^50."""
    d, e = R.scaled_tridiag(kind, n, rung)
    d64, e64 = d.astype(np.float64), e.astype(np.float64)
    T = np.diag(d64) + np.diag(e64, 1) + np.diag(e64, -1)
    ref_w = np.linalg.eigvalsh(T)   # (dense fp64 LAPACK: stemr of scipy.linalg.eigh_tridiagonal gives up at 2^50, n = 500)
    scale = np.abs(ref_w).max()
    dd, ee = torch.from_numpy(d).to(C.DEV), torch.from_numpy(e).to(C.DEV)
    w, _ = kernels.stedc(dd, ee, eigenvectors=False)
    err0 = np.abs(w.cpu().double().numpy() - ref_w).max()
    w, Z = kernels.stedc(dd, ee, eigenvectors=True)
    wc, Zc = w.cpu().double().numpy(), Z.cpu().double().numpy()
    err1, orth, resid = np.abs(wc - ref_w).max(), np.abs(Zc.T @ Zc - np.eye(n)).max(), np.abs(T @ Zc - Zc * wc[None, :]).max()
    print(f"stedc {kind} n={n} rung={rung}: values {err0 / scale:.3e}  with vectors {err1 / scale:.3e}  orth {orth:.3e}  "
          f"resid {resid / scale:.3e}")
    assert np.isfinite(wc).all() and np.isfinite(Zc).all()
    assert err0 <= 1e-6 * scale
    assert err1 <= 2e-6 * scale
    assert orth < 1e-5
    assert resid <= 5e-6 * scale
