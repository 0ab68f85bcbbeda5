"""The output side and the workspace of every route of the public GEMMs and the Gram SYRK (tests/gemm_output_child.py).

Every other GEMM test writes a contiguous `out` (ldc == N) through the wrappers, whose workspace is 1.25 x the query + 256
bytes.  Here `out` is a window of NaN-filled storage (ldc = N + 7, C four bytes off a 16-byte boundary: what
_gemm_nt_within, _slab_of_gs and the sequence closures hand the library), beta = 0 runs over a window left NaN, and the
workspace is a slice of pattern-filled memory of EXACTLY the query's bytes -- or fewer: the last column of the route table
in csrc/gemm_plan.h (Tile256Bx falls back to Tile256, Tile256 takes the splits that fit, BxSplitK is skipped, the rest
return VIVIT_E_WORKSPACE with nothing written).  One child process per environment, since the route switches are read once
per process: the default routes, and VIVIT_GEMM_SPLIT=0 (gemm256_kernel itself, where the re-plan to fewer splits runs).  A
child that ends on a signal or its time limit fails its test at once; nothing is started after it.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_TIMEOUT = 240   # seconds: some sixty products of at most 0.3 TFLOP with their fp64 references, after the start of the process
_RESULTS = {}


def _child(mode, tmp_path_factory):
    """(exit status, log, {case: "ok" | text}, {name: digest}) of the child process of `mode`, run once."""
    if mode not in _RESULTS:
        import gemm_output_child as C   # (the list of cases; nothing runs on import but the library load)

        tmp = tmp_path_factory.mktemp(f"gemm_output_{mode}")
        out, dig = tmp / "out.json", tmp / "digests.json"
        env = {k: v for k, v in os.environ.items() if k != "VIVIT_GEMM_SPLIT"}
        env.update(C.MODES[mode])
        proc = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.join(HERE, "gemm_output_child.py"), mode,
                               str(out), str(dig)], env=env, cwd=HERE, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        _RESULTS[mode] = (proc.returncode, proc.stdout, json.loads(out.read_text()) if out.exists() else {},
                          json.loads(dig.read_text()) if dig.exists() else {})
    return _RESULTS[mode]


@pytest.mark.parametrize("mode", ["default", "split0"])
def test_outputs_and_workspaces(mode, tmp_path_factory):
    """Exact workspace, output window, fp64 bound, K == 0 and the shorter workspaces of every case of the child."""
    import gemm_output_child as C

    status, log, res, _ = _child(mode, tmp_path_factory)
    print(log[-6000:])
    assert status == 0, f"child ended with status {status} after {list(res)}"
    bad = {k: v for k, v in res.items() if v != "ok"}
    assert not bad, bad
    assert list(res) == [name for name, _ in C.jobs(mode)]


@pytest.mark.parametrize("case", ["tile256-nt", "tile256-syrk"])
def test_null_workspace_runs_the_fp32_kernel(case, tmp_path_factory):
    """Without a workspace the bf16 pipe of the 256 tile falls back to gemm256_kernel with one split: the bytes of the
    VIVIT_GEMM_SPLIT=0 process (the same kernel), and not those of the default process on the whole query (the child of
    `default` compares these two itself)."""
    runs = {mode: _child(mode, tmp_path_factory) for mode in ("default", "split0")}
    for mode, (status, _, res, _) in runs.items():
        assert status == 0 and res.get(f"null-{case}") == "ok", (mode, status, res.get(f"null-{case}"))
    assert runs["default"][3][f"{case}-null"] == runs["split0"][3][f"{case}-null"]
