"""The cross-entropy factor with a scale per position (``vivit_ce_target_scales_f32`` + ``vivit_ce_pos_sqrt_hessian_w_f32``) against the
unweighted entry point (``vivit_ce_pos_sqrt_hessian_f32``) in ONE process on the same tensors, in the manner of loss_positions_ab.py:
sampled factor, M = 1, at the two shapes DESIGN.md reports for the unweighted kernel.

Three contenders per shape, called in turn (the order reversed in odd rounds), 40 timed rounds after 3 warm-ups of each, device events
around one call (for the weighted ones: the two launches of the scales and the factor launch):

* ``plain``     the unweighted entry point with ``scale = 1 / sqrt(N L)``;
* ``weighted``  the scales from targets of which none is ignored, then the factor -- must give the bytes of ``plain``;
* ``padded``    the same with the second half of every sample's positions at ``ignore_index`` (right padding).

Per contender: median, minimum, quartiles and maximum, and the medians of the first and second half of the rounds (drift).

    python scripts/probe/loss_weighted_time.py [--out FILE]
"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from vivit_amd import kernels                                        # noqa: E402


def case(title, N, C, D, classes_last, lines, rounds=40):
    dev = torch.device("cuda:0")
    L = math.prod(D)
    if classes_last:
        z = torch.randn((N,) + D + (C,), device=dev).movedim(-1, 1)
    else:
        z = torch.randn((N, C) + D, device=dev)
    idx = torch.randint(0, C, (1, N) + D, device=dev, dtype=torch.int32)
    y = torch.randint(0, C, (N,) + D, device=dev)
    y_pad = y.clone()
    y_pad.view(N, L)[:, L // 2:] = -100
    scale = 1.0 / math.sqrt(N * L)

    calls = {
        "plain": lambda: kernels.ce_sqrt_hessian_positions(z, scale, idx=idx),
        "weighted": lambda: kernels.ce_sqrt_hessian_positions_w(z, kernels.ce_target_scales(y, C), idx=idx),
        "padded": lambda: kernels.ce_sqrt_hessian_positions_w(z, kernels.ce_target_scales(y_pad, C), idx=idx),
    }
    names = list(calls)
    same = torch.equal(calls["plain"](), calls["weighted"]())
    for k in names:
        for _ in range(3):
            calls[k]()
    torch.cuda.synchronize()
    times = {k: [] for k in names}
    for r in range(rounds):
        for k in (names if r % 2 == 0 else names[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            S = calls[k]()
            b.record()
            b.synchronize()
            del S
            times[k].append(a.elapsed_time(b))
    for k in names:
        t = sorted(times[k])
        halves = (statistics.median(times[k][:rounds // 2]), statistics.median(times[k][rounds // 2:]))
        lines.append(f"{title} {k:8s}: median {statistics.median(t):.4f} ms, min {t[0]:.4f}, quartiles {t[len(t) // 4]:.4f} / "
                     f"{t[3 * len(t) // 4]:.4f}, max {t[-1]:.4f}; medians of the first / second {rounds // 2} rounds {halves[0]:.4f} / "
                     f"{halves[1]:.4f}")
    lines.append(f"{title}: weighted (nothing ignored) and plain give the same bytes: {same}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this probe measures on the GPU: none found")
    torch.manual_seed(0)
    lines = []
    case("NLC [64, 32000, 128]", 64, 32000, (128,), True, lines)
    case("NCL [16, 21, 128, 128]", 16, 21, (128, 128), False, lines)
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
