"""Child of tests/test_symeigh_batched_gpu.py: batched and single two-phase reductions under the environment knobs of the
parent (they are read once per process).  Writes {"n:B": {"batched": [...], "single": [...], "state": [...],
"single_select": [...]}}: hex of the eigenvalues per problem, and of ``plans[b].select(top 10)`` (the single select on the
batched reduction's state) against ``symeig_reduce(G_b).select(top 10)``."""
import json
import sys

import torch

from helpers import ROOT  # noqa: F401  (puts the repository root on sys.path)
from symeig_batched_child import batch_inputs, hexes
from vivit_amd import kernels

CASES = [(193, 3), (256, 8), (777, 3), (1024, 11), (1280, 8)]


def main(out):
    dev = torch.device("cuda:0")
    res = {}
    for n, B in CASES:
        mats = batch_inputs(n, B, dev)
        keep = list(range(n - 10, n))
        bp = kernels.symeig_reduce_batched(mats)
        singles = [kernels.symeig_reduce(G) for G in mats]
        res[f"{n}:{B}"] = {"batched": hexes(bp.evals), "single": hexes([p.evals for p in singles]),
                           "state": hexes([p.select(keep) for p in bp.plans]),
                           "single_select": hexes([p.select(keep) for p in singles])}
    torch.cuda.synchronize()
    with open(out, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1])
