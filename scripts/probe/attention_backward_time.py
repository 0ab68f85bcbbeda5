"""Time the backward pass of scaled dot-product self-attention alone, on one MI355X, in one process, the two paths alternating per
shape:

    (a) ``kernels.attention_jac_t(dout[None], ...)``: the rule on the gradient as a factor of one row -- the backward pass behind
        ``fused_forward=True`` before csrc/attention_backward.hip existed, with its lse and row-dot launches;
    (b) ``kernels.attention_backward(dout, ..., lse)``: the one-row kernels that reuse the forward's lse.

Shapes: the three of scripts/probe/attention_forward_time.py (12 heads of 64) and H = 32, d = 128, T = 2048, N = 2 without a mask.  Per
shape the largest difference between the two results, then the times; then, as the forward probe prints it, the modules' forward +
backward with ``fused_forward=False`` (the torch formula) and ``True``.  Device events, 20 calls after 3 warm-ups: median, minimum and
maximum.  The last line of a shape says whether the whole range of (b) lies below that of (a).

The work is done in a child process under ``timeout``; after a child that fails or runs out of time nothing more is started.

    python scripts/probe/attention_backward_time.py [--out FILE]
"""
import argparse
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from attention_scoremod_time import fmt, timed   # noqa: E402

SHAPES = [(12, 64, 512, 8, False, False), (12, 64, 2048, 4, False, False), (12, 64, 2048, 4, True, True),
          (32, 128, 2048, 2, False, False)]   # (H, d, T, N, causal, half padded)
STEP_SECONDS = 400


def run():
    from vivit_amd import kernels
    from vivit_amd.backend import ScaledDotProductAttention

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lines = []
    for H, D, T, N, causal, padded in SHAPES:
        scale = D ** -0.5
        x, dout = torch.randn(N, T, 3 * H * D, device=dev), torch.randn(N, T, H * D, device=dev)
        lengths = torch.full((N,), T // 2, dtype=torch.int32, device=dev) if padded else None
        lines.append(f"H={H}, d={D}, T={T}, N={N}, causal={causal}, lengths={'T / 2' if padded else 'none'}")
        out, lse = kernels.attention_forward(x, H, scale, causal, lengths=lengths, return_lse=True)
        rule = lambda: kernels.attention_jac_t(dout[None], x, out, H, scale, causal, lengths=lengths)[0]   # noqa: E731
        back = lambda: kernels.attention_backward(dout, x, out, lse, H, scale, causal, lengths=lengths)   # noqa: E731
        lines.append(f"  largest difference between the two results: {(rule() - back()).abs().max().item():.3g}")
        t_a, t_b = timed(rule), timed(back)
        lines.append(fmt("(a) backward alone, attention_jac_t on one row ", t_a))
        lines.append(fmt("(b) backward alone, attention_backward        ", t_b) + f"  (a) / (b) = {t_a[0] / t_b[0]:.2f}")
        lines.append(f"  the range of (b) lies wholly below that of (a): {t_b[2] < t_a[1]}")
        modules = {}
        for fused in (False, True):
            modules[fused] = ScaledDotProductAttention(H, causal=causal, fused_forward=fused).to(dev)
            modules[fused].set_lengths(lengths)

        def both(fused):
            xg = x.detach().requires_grad_()
            modules[fused](xg).sum().backward()
            return xg.grad

        lines.append(f"  largest difference between the modules' input gradients: {(both(True) - both(False)).abs().max().item():.3g}")
        times = {fused: timed(lambda: both(fused)) for fused in (False, True)}
        lines.append(fmt("module forward + backward fused_forward=False", times[False]))
        lines.append(fmt("module forward + backward fused_forward=True ", times[True]) + f"  torch / fused = {times[False][0] / times[True][0]:.2f}")
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
