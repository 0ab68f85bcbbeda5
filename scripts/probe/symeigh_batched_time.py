"""Eight eigenpair solves of one size (top 10 eigenvectors each): eight consecutive ``kernels.symeig_reduce`` + ``select``
against one ``kernels.symeig_reduce_batched`` + ``select``.

    python scripts/probe/symeigh_batched_time.py --mode seq      [--sizes 256 1024 1280] [--reps 20] [--warmup 3]
    python scripts/probe/symeigh_batched_time.py --mode batched  ...
    python scripts/probe/symeigh_batched_time.py --mode vals     (eight values-only solves through kernels.symeigvals_batched)
    python scripts/probe/symeigh_batched_time.py --mode api      (12 single-parameter groups, N C = 1280, batched_solve off / on)

``--mode seq`` and ``--mode vals`` use nothing this change adds, so the same script run with ``--root`` pointing at a
checkout of an older commit times that commit's library: that is the same-box A/B.  Protocol of
scripts/probe/symeig_batched_time.py: a timed region is bracketed by events on the stream and holds only the solves (the
inputs are restored outside it); reported per size: median, min, max of the repetitions, one JSON line each."""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=["seq", "batched", "vals", "api"], required=True)
ap.add_argument("--sizes", type=int, nargs="+", default=[256, 1024, 1280])
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--topk", type=int, default=10)
ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."),
                help="checkout whose vivit_amd is timed (default: this one)")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402

from vivit_amd import kernels  # noqa: E402

DEV = torch.device("cuda:0")


def inputs(n, B=8):
    mats = []
    for i in range(B):
        g = torch.Generator().manual_seed(1000 * n + i)
        V = torch.randn(n, 2 * n, generator=g) / n ** 0.5
        mats.append((V @ V.T).to(DEV))
    return mats


def timed(fn, restore, reps, warmup):
    times = []
    for r in range(warmup + reps):
        restore()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if r >= warmup:
            times.append(a.elapsed_time(b))
    return times


def report(tag, n, times):
    print(json.dumps({"what": tag, "n": n, "reps": len(times), "median_ms": round(statistics.median(times), 4),
                      "min_ms": round(min(times), 4), "max_ms": round(max(times), 4)}), flush=True)


def solves():
    for n in args.sizes:
        keep = inputs(n)
        work = [G.clone() for G in keep]
        top = list(range(n - args.topk, n))

        def restore():
            for w, k in zip(work, keep):
                w.copy_(k)

        if args.mode == "seq":
            def fn():
                return [kernels.symeig_reduce(w, overwrite=True).select(top) for w in work]
        elif args.mode == "vals":
            def fn():
                return kernels.symeigvals_batched(work, overwrite=True)
        else:
            def fn():
                return kernels.symeig_reduce_batched(work, overwrite=True).select([top] * len(work))
        report(args.mode, n, timed(fn, restore, args.reps, args.warmup))


def api():
    from torch import nn

    import vivit_amd
    from vivit_amd.backend import backpack, extend

    torch.manual_seed(0)
    C, N = 10, 128
    layers = []
    for i in range(12):
        layers += [nn.Linear(C, C, bias=False)] + ([nn.Tanh()] if i < 11 else [])
    model = extend(nn.Sequential(*layers).to(DEV))
    lossf = extend(nn.CrossEntropyLoss())
    X, y = torch.rand(N, C, device=DEV), torch.randint(0, C, (N,), device=DEV)

    def criterion(evals):
        return list(range(evals.numel() - 6, evals.numel()))

    for batched in (False, True):
        def fn():
            comp = vivit_amd.EighComputation(batched_solve=batched, warn_small_eigvals=0.0)
            groups = [{"params": [p], "criterion": criterion} for p in model.parameters()]
            model.zero_grad()
            loss = lossf(model(X), y)
            with backpack(comp.get_extension(), extension_hook=comp.get_extension_hook(groups)):
                loss.backward()
            return [comp.get_result(g) for g in groups]

        report(f"api12 eigh batched_solve={batched}", N * C, timed(fn, lambda: None, args.reps, args.warmup))


if __name__ == "__main__":
    api() if args.mode == "api" else solves()
