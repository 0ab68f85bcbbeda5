"""Child of tests/test_symeig_batched_gpu.py: batched and single eigenvalue solves under the environment knobs of the
parent (they are read once per process).  Writes {"n:B": {"batched": [hex per problem], "single": [hex per problem]}}."""
import json
import sys

import torch

from helpers import ROOT  # noqa: F401  (puts the repository root on sys.path)
from vivit_amd import kernels

CASES = [(193, 3), (256, 8), (300, 11), (777, 3), (1024, 8), (1280, 11)]


def batch_inputs(n, B, dev):
    """B seeded symmetric matrices M + M^T, the last one replaced by a rank-deficient PSD Gram matrix (rank n // 3)."""
    mats = []
    for i in range(B):
        g = torch.Generator().manual_seed(1000 * n + i)
        if i == B - 1:
            V = torch.randn(n, max(n // 3, 1), generator=g)
            mats.append((V @ V.T).to(dev))
        else:
            M = torch.randn(n, n, generator=g)
            mats.append((M + M.T).to(dev))
    return mats


def hexes(W):
    return [row.cpu().numpy().tobytes().hex() for row in W]


def main(out):
    dev = torch.device("cuda:0")
    res = {}
    for n, B in CASES:
        mats = batch_inputs(n, B, dev)
        W = kernels.symeigvals_batched(mats)
        S = torch.stack([kernels.symeig(G, eigenvectors=False)[0] for G in mats])
        res[f"{n}:{B}"] = {"batched": hexes(W), "single": hexes(S)}
    torch.cuda.synchronize()
    with open(out, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1])
