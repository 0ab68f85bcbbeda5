"""Every eigensolver entry of the C ABI on exactly the bytes its workspace query asks for (tests/eig_workspace_exact_child.py).

The Python wrappers allocate 1.25 x the query + 256 bytes, so nothing else in the suite notices a query that forgets a
buffer or a layout that grows past it.  Here each workspace is a slice of a pattern-filled buffer, misaligned by 16 bytes
and exactly ``query`` long; after the call the pattern on both sides must be intact and the outputs byte-equal to the
wrapper's.  Three child processes, one per set of layouts: the default routes (persistent one-stage reduction at n = 200 and
300, the batched waves), the two-stage layouts forced at the same sizes, and the launch chains with the persistent kernels
off.  A child that ends on a signal or its time limit fails the test at once; nothing is started after it.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
HERE = os.path.dirname(os.path.abspath(__file__))
ENVS = {"default": {}, "two_stage": {"VIVIT_TWO_STAGE": "1"},
        "launch_chains": {"VIVIT_SYTRD_PERSIST": "0", "VIVIT_QR_PERSIST": "0", "VIVIT_SB2ST_PERSIST": "0"}}
CHILD_TIMEOUT = 180   # seconds: twelve cases of a few seconds each after the start of the process


@pytest.mark.parametrize("key", list(ENVS))
def test_every_entry_on_exactly_its_query(key, tmp_path):
    import eig_workspace_exact_child as C   # (the list of cases; nothing runs on import but the library load)

    out = tmp_path / "out.json"
    env = {k: v for k, v in os.environ.items() if k not in ("VIVIT_TWO_STAGE", "VIVIT_SYTRD_PERSIST", "VIVIT_QR_PERSIST", "VIVIT_SB2ST_PERSIST")}
    env.update(ENVS[key])
    proc = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.join(HERE, "eig_workspace_exact_child.py"), str(out)],
                          env=env, cwd=HERE, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(proc.stdout[-4000:])
    res = json.loads(out.read_text()) if out.exists() else {}
    assert proc.returncode == 0, f"child ended with status {proc.returncode} after {list(res)}"
    bad = {k: v for k, v in res.items() if v != "ok"}
    assert not bad, bad
    assert list(res) == [name for name, _ in C.CASES]
