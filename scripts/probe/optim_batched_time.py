"""A damped-Newton sweep over per-layer groups of one Gram size, ``batched_solve`` off against on, in one process.

    python scripts/probe/optim_batched_time.py [--groups 8 12] [--reps 20] [--warmup 3] [--topk 10]

The factors (n = C N = 1280, P = 256 per group; tests/helpers.planted_factors rule: ten planted directions above the bulk)
are on the device before the clock starts; the timed region runs from the group hooks -- Gram build, ``V^T g``, the
eigensolves, gammas / lambdas, the damping callback, the back-projection -- to the last ``get_result``.  It is bracketed by
events on the stream; the two modes alternate repetition by repetition, so drift hits both alike.  Reported per workload
and mode: median, min, max, one JSON line each, then the ratio of the medians.  The baseline (``batched_solve=False``) is
the path the computations always had."""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--groups", type=int, nargs="+", default=[8, 12])
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--topk", type=int, default=10)
args = ap.parse_args()
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import vivit_amd  # noqa: E402

DEV = torch.device("cuda:0")
C, N, P = 10, 128, 256


class Leaf(torch.nn.Module):
    """What the group hooks need of a module: its parameters and ``input0`` (the batch size)."""

    def __init__(self, params):
        super().__init__()
        for i, p in enumerate(params):
            self.register_parameter(f"p{i}", p)
        self.input0 = torch.zeros(N, 1)


def factors(i):
    g = torch.Generator().manual_seed(100 + i)
    V = torch.randn(C, N, P, generator=g) / N ** 0.5
    G = torch.randn(N, P, generator=g) / N
    for j in range(10):
        u, w = torch.randn(C, N, generator=g), torch.randn(P, generator=g)
        V += (100.0 * 1.5 ** j) ** 0.5 * (u / u.norm()).reshape(C, N, 1) * (w / w.norm())
    return V.to(DEV), G.to(DEV)


def criterion(evals):
    return list(range(evals.numel() - args.topk, evals.numel()))


def damping(evals, evecs, gammas, lambdas):
    return torch.ones_like(evals)


def sweep(VG, batched):
    comp = vivit_amd.DirectionalDampedNewtonComputation(warn_small_eigvals=0.0, batched_solve=batched)
    params = [torch.nn.Parameter(torch.zeros(P, device=DEV)) for _ in VG]
    for p, (V, G) in zip(params, VG):     # views: attaching costs nothing and the hooks do not modify the factors
        setattr(p, comp._savefield_ggn, V)
        setattr(p, comp._savefield_grad, G)
    groups = [{"params": [p], "criterion": criterion, "damping": damping} for p in params]
    module = Leaf(params)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    comp.get_extension_hook(groups)(module)
    steps = [comp.get_result(g) for g in groups]
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), steps


def main():
    for count in args.groups:
        VG = [factors(i) for i in range(count)]
        times = {False: [], True: []}
        for r in range(args.warmup + args.reps):
            for batched in (False, True):
                ms, _ = sweep(VG, batched)
                if r >= args.warmup:
                    times[batched].append(ms)
        med = {}
        for batched in (False, True):
            t = times[batched]
            med[batched] = statistics.median(t)
            print(json.dumps({"what": f"newton sweep, {count} groups, batched_solve={batched}", "n": C * N, "reps": len(t),
                              "median_ms": round(med[batched], 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}),
                  flush=True)
        print(json.dumps({"what": f"newton sweep, {count} groups", "immediate_over_batched": round(med[False] / med[True], 3)}),
              flush=True)


if __name__ == "__main__":
    main()
