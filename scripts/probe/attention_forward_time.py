"""Time the forward pass of ``ScaledDotProductAttention`` with ``fused_forward=False`` (the torch formula) and ``True`` (the flash-style
kernel of csrc/attention_forward.hip; autograd's backward pass is then the rule's kernels) on one MI355X, in one process, the two
alternating per shape: 12 heads of 64,

    (1) T = 512,  N = 8, no mask
    (2) T = 2048, N = 4, no mask
    (3) T = 2048, N = 4, causal, half of every sequence padded (lengths = T / 2)

and per shape and path the forward time, the forward + backward time (``out.sum().backward()``) and the peak memory beyond the input.
Device events, 20 calls after 3 warm-ups: median, minimum and maximum.  Before anything is timed the two outputs and the two input
gradients of each shape are compared.

The work is done in a child process under ``timeout``; after a child that fails or runs out of time nothing more is started.

    python scripts/probe/attention_forward_time.py [--out FILE]
"""
import argparse
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from attention_scoremod_time import fmt, peak_extra, timed   # noqa: E402

H, D = 12, 64
SHAPES = [(512, 8, False, False), (2048, 4, False, False), (2048, 4, True, True)]   # (T, N, causal, half padded)
STEP_SECONDS = 400


def run():
    from vivit_amd.backend import ScaledDotProductAttention

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lines = []
    for T, N, causal, padded in SHAPES:
        x = torch.randn(N, T, 3 * H * D, device=dev)
        lines.append(f"H={H}, d={D}, T={T}, N={N}, causal={causal}, lengths={'T / 2' if padded else 'none'}; one fp32 [N, H, T, T] is "
                     f"{N * H * T * T * 4 / 2 ** 20:.0f} MiB, input + output {N * T * 4 * H * D * 4 / 2 ** 20:.0f} MiB")
        modules = {}
        for fused in (False, True):
            modules[fused] = ScaledDotProductAttention(H, causal=causal, fused_forward=fused).to(dev)
            modules[fused].set_lengths(torch.full((N,), T // 2, dtype=torch.int32, device=dev) if padded else None)

        def forward(fused):
            with torch.no_grad():
                return modules[fused](x)

        def both(fused):
            xg = x.detach().requires_grad_()
            modules[fused](xg).sum().backward()
            return xg.grad

        diff_o = (forward(True) - forward(False)).abs().max().item()
        diff_g = (both(True) - both(False)).abs().max().item()
        lines.append(f"  largest difference between the two paths: output {diff_o:.3g}, input gradient {diff_g:.3g}")
        times = {}
        for name, fn in (("forward", forward), ("forward + backward", both)):
            for fused in (False, True):
                times[name, fused] = timed(lambda: fn(fused))
                lines.append(fmt(f"{name:18s} fused_forward={fused!s:5s}", times[name, fused])
                             + (f"  torch / fused = {times[name, False][0] / times[name, True][0]:.2f}" if fused else ""))
        for name, fn in (("forward", forward), ("forward + backward", both)):
            lines.append(f"  peak memory beyond the input, {name}: torch {peak_extra(lambda: fn(False)) / 2 ** 20:.1f} MiB, "
                         f"fused {peak_extra(lambda: fn(True)) / 2 ** 20:.1f} MiB")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the lines to this file")
    ap.add_argument("--child", action="store_true", help="(internal) do the work in this process")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    if args.child:
        print("\n".join(run()))
        return 0
    child = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--child"],
                           stdout=subprocess.PIPE, text=True)
    text = child.stdout.rstrip("\n")
    if child.returncode != 0:
        text += f"\nexit status {child.returncode}; nothing more was started"
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")
    return child.returncode


if __name__ == "__main__":
    sys.exit(main())
