"""Every route of the symmetric eigensolver on degenerate matrices, at scale 1 and at 2^-100.

The zero matrix, c I, a diagonal and an already tridiagonal matrix (every reflector degenerate, tau = 0), an exactly
block-diagonal matrix (e exactly 0 at a split; n = 260 puts the split inside a panel of 64 on the persistent route), a Gram
matrix with a dead sample, rank one, a negative semidefinite matrix, the antidiagonal (two eigenvalues, each n / 2 times) and
an arrowhead (tests/eig_edge_refs.py::degenerate).  ``check_eigen`` holds every result to the suite's bounds and, for c I and
diagonal input, to exactness; a route whose ``info`` is not 0 raises, and a NaN in any output fails the check.

One test case runs one (route, kind, size) at both scales and names every scale that fails.  Routes chosen by
``VIVIT_TWO_STAGE`` run in ONE child process for all their cases (tests/symeig_scale_child.py)."""
import pytest

import eig_edge_refs as R
import symeig_scale_child as C
from test_symeig_scale_gpu import assert_child_cases, case_id, run_child

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
SCALES = (0, -100)

IN_PROCESS = [("full", 33), ("full", 192), ("full", 200), ("chain", 200), ("rows", 200), ("band", 200), ("select", 200),
              ("select_dc", 260)]
TWO_STAGE = [("full", 200), ("rows", 200), ("select", 200)]
BATCHES = [R.DEGENERATE[i:i + 3] for i in (0, 3, 6)] + [("arrowhead", "zero", "dead_sample")]


def expand(table):
    out = [(route, kind, n) for route, n in table for kind in R.DEGENERATE]
    out += [("full", "blockdiag", 260)] if ("full", 200) in table else []
    out += [("select_cluster", "antidiag", 200)]   # all of one cluster: only the eigenspace is defined
    return out


@pytest.mark.parametrize("route,kind,n", expand(IN_PROCESS), ids=[case_id(c) for c in expand(IN_PROCESS)])
def test_degenerate_input(route, kind, n):
    C.check_all(route, [(f"2^{s}", [R.degenerate(kind, n, s)], [kind]) for s in SCALES])


@pytest.mark.parametrize("kinds", BATCHES, ids=[case_id(c) for c in BATCHES])
@pytest.mark.parametrize("route,n", [("batched_values", 64), ("batched_values", 200), ("batched_select", 200)])
def test_batch_of_degenerate_inputs(route, n, kinds):
    """Three different degenerate problems in one launch: each checked, each byte-identical to its single solve."""
    C.check_all(route, [(f"2^{s}", [R.degenerate(kind, n, s) for kind in kinds], kinds) for s in SCALES])


TWO_STAGE_GROUPS = expand(TWO_STAGE)
TWO_STAGE_CASES = [{"id": case_id(c + (s,)), "fn": "route", "route": c[0], "inputs": [["degenerate", c[1], c[2], s]]}
                   for c in TWO_STAGE_GROUPS for s in SCALES]


@pytest.fixture(scope="module")
def two_stage(tmp_path_factory):
    return run_child(tmp_path_factory.mktemp("degenerate"), "two_stage", TWO_STAGE_CASES, VIVIT_TWO_STAGE="1")


@pytest.mark.parametrize("route,kind,n", TWO_STAGE_GROUPS, ids=[case_id(c) for c in TWO_STAGE_GROUPS])
def test_degenerate_input_two_stage(two_stage, route, kind, n):
    assert_child_cases(two_stage, [case_id((route, kind, n, s)) for s in SCALES])
