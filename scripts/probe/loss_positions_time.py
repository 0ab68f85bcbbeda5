"""Time the sampled per-position cross-entropy factor (csrc/loss_positions.hip, ``kernels.ce_sqrt_hessian_positions``) on one MI355X
against the torch composition on the same device tensors in the same run -- what the rule's non-kernel path computes
(``_loss_hessian_sqrt_positions`` of vivit_amd/backend/extensions.py): ``softmax`` over the classes, ``one_hot`` of the indices, the
difference, the scale, and the copy into the memory format the layer below reads (a no-op where the composition already has it).

Shapes, both with M = 1 sampled slice:
  * language model, NLC: logits ``[N, C, T] = [64, 32 000, 128]`` as ``Permute(0, 2, 1)`` hands them over (a view of a contiguous
    ``[N, T, C]``); the head below wants the factor as a contiguous ``[M, N, T, C]``;
  * segmentation, NCL: logits ``[N, C, H, W] = [16, 21, 128, 128]`` contiguous; the convolution below wants ``[M, N, C, H, W]``.

Per shape and route: median, minimum and maximum of the timed calls (device events around one call, launches included: a call time,
not a kernel time from a trace; 2 warm-ups of each route, then 10 rounds that call every route once, in turn, so that drift and other
work on the machine meet them alike), the algorithmic bytes per second of the median against the 8 TB/s specification, the peak device
memory of one call above the operands, and max |difference| / max |reference| between the routes.

Bytes counted: the logits read once, the M slices of the factor written once (the indices, 1 / C of that, are not counted).

    python scripts/probe/loss_positions_time.py [--out FILE]
"""
import argparse
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from vivit_amd import kernels                                        # noqa: E402

HBM_PEAK = 8.0e12           # bytes/s, specification
MIB = 2.0 ** 20
M = 1


def one_call(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    res = fn()
    t1.record()
    t1.synchronize()
    del res
    return t0.elapsed_time(t1) * 1e-3


def timed_alternating(fns, warm=2, rounds=10):
    """{name: sorted call times}: ``warm`` calls of each, then rounds that call every function once, in turn."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(one_call(fn))
    return {name: sorted(t) for name, t in times.items()}


def peak_above_base(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del res
    return peak


def report(title, nbytes, fns, reference):
    times = timed_alternating(fns)
    ref = fns[reference]()
    lines = [title]
    for name, fn in fns.items():
        t = times[name]
        med = statistics.median(t)
        err = ((fn() - ref).abs().max() / ref.abs().max()).item()
        lines.append(f"  {name:<20s} median {med * 1e3:9.3f} ms (min {t[0] * 1e3:9.3f}, max {t[-1] * 1e3:9.3f})  "
                     f"{nbytes / med / 1e12:5.2f} TB/s = {100 * nbytes / med / HBM_PEAK:4.1f} % of 8 TB/s  "
                     f"peak memory above the operands {peak_above_base(fn) / MIB:9.1f} MiB  max |diff| / max |{reference}| {err:.2e}")
    lines.append(f"  bytes counted: {nbytes / 1e9:.3f} GB")
    print("\n".join(lines), flush=True)
    return lines


def case(title, logits, classes_last):
    """``logits [N, C, *D]`` (a permuted view when ``classes_last``); both routes return the factor in the layout the layer below
    reads: ``[M, N, *D, C]`` contiguous when ``classes_last``, ``[M, N, C, *D]`` contiguous otherwise."""
    N, C, D = logits.shape[0], logits.shape[1], tuple(logits.shape[2:])
    L = math.prod(D)
    scale = 1.0 / math.sqrt(M * N * L)
    idx = torch.multinomial(logits.softmax(1).movedim(1, -1).reshape(N * L, C), M, replacement=True).t().reshape(M, N, *D)
    idx32 = idx.to(torch.int32)

    def below(S):
        out = (S.movedim(2, -1) if classes_last else S).contiguous()
        assert out.is_contiguous()
        return out

    def hip():
        return below(kernels.ce_sqrt_hessian_positions(logits, scale, idx=idx32))

    def composition():
        onehot = F.one_hot(idx, C).movedim(-1, 2).to(logits.dtype)
        return below((logits.softmax(dim=1).unsqueeze(0) - onehot) * scale)

    return report(title, 4 * (1 + M) * logits.numel(), {"HIP kernel": hip, "torch composition": composition}, "torch composition")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this probe measures on the GPU: none found")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lines = [f"{torch.cuda.get_device_name(0)}; call times by device events, 10 alternating rounds after 2 warm-ups of each route"]
    N, T, C = 64, 128, 32000
    lines += case(f"sampled CE factor, NLC: logits [N={N}, C={C}, T={T}] (a view of [N, T, C]), M = {M}",
                  torch.randn(N, T, C, device=dev).permute(0, 2, 1), True)
    torch.cuda.empty_cache()
    N, C, H, W = 16, 21, 128, 128
    lines += case(f"sampled CE factor, NCL: logits [N={N}, C={C}, {H}, {W}] contiguous, M = {M}", torch.randn(N, C, H, W, device=dev), False)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
