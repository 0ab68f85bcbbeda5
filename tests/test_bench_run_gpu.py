"""bench.py end to end on the small BASELINE config 1 workload (n = 1280): a plain run prints the headline line and nothing
it does not need; ``--full`` adds the parity check and the secondary lines of the same run."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
EXTRA_KEYS = ("verified", "secondary", "configs", "cpu_baseline")


def _bench(*flags):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "mlp784-512-10_b128", *flags]
    proc = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-4000:]
    lines = proc.stdout.strip().splitlines()
    assert len(lines) == 1, proc.stdout[-4000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_only_the_headline(tmp_path):
    out = _bench("--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert all(k in out for k in HEADLINE_KEYS), out
    assert (out["steps"], out["warmup"], out["extras"]) == (2, 1, [])
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["unit"] == "eigenpairs/s" and out["higher_is_better"] is True
    assert not any(k in out for k in EXTRA_KEYS), sorted(out)
    assert sorted(os.listdir(tmp_path)) == ["eigenvalues.npy", "eigenvector_columns.npy", "eigenvectors.npy"]


@pytest.mark.gpu
def test_full_run_adds_the_extras():
    out = _bench("--steps", "1", "--warmup", "1", "--full", "--no-configs", "--no-cpu-baseline")
    assert all(k in out for k in HEADLINE_KEYS), out
    assert out["extras"] == ["secondary", "verify"]
    assert out["verified"]["ok"] is True, out["verified"]
    assert "eigvalsh_s" in out["secondary"] and "api_error" not in out["secondary"], out["secondary"]
    assert "configs" not in out and "cpu_baseline" not in out
