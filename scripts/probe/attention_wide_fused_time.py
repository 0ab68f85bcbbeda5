"""Time scaled dot-product self-attention at head dimensions 129 to 256 on one MI355X, in one process, the paths of each comparison
one after the other per shape:

    (a) the forward pass alone (no autograd): the module with ``fused_forward=False`` -- the torch formula, what ran at this width
        before csrc/attention_wide_forward.hip existed -- against ``True`` (``kernels.attention_wide_forward``);
    (b) the backward pass alone: ``kernels.attention_wide_jac_t(dout[None], ...)``, the rule on the gradient as a factor of one row,
        against ``kernels.attention_wide_backward(dout, ..., lse)``, the one-row kernels that reuse the forward's lse;
    (c) the modules' forward + backward, torch autograd against ``fused_forward=True``, with the peak memory beyond the input.

Shapes: 8 query heads of 256 over 4 key / value heads and 8 heads of 192, T = 512 and T = 2048 without a mask, and the first at
T = 2048 causal with half of every sequence padded.  Per shape the largest differences between the paths' results, then the times.
Device events, 20 calls after 3 warm-ups: median, minimum and maximum.  The last line of (b) says whether its whole range lies below
the rule's.

The work is done in a child process under ``timeout``; after a child that fails or runs out of time nothing more is started.

    python scripts/probe/attention_wide_fused_time.py [--out FILE]
"""
import argparse
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from attention_scoremod_time import fmt, peak_extra, timed   # noqa: E402

SHAPES = [(8, 4, 256, 512, 4, False, False), (8, 4, 256, 2048, 2, False, False), (8, 8, 192, 512, 4, False, False),
          (8, 8, 192, 2048, 2, False, False), (8, 4, 256, 2048, 2, True, True)]   # (H, Hkv, d, T, N, causal, half padded)
STEP_SECONDS = 400


def run():
    from vivit_amd import kernels
    from vivit_amd.backend import ScaledDotProductAttention

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lines = []
    for H, Hkv, D, T, N, causal, padded in SHAPES:
        scale = D ** -0.5
        x, dout = torch.randn(N, T, (H + 2 * Hkv) * D, device=dev), torch.randn(N, T, H * D, device=dev)
        lengths = torch.full((N,), T // 2, dtype=torch.int32, device=dev) if padded else None
        lines.append(f"H={H}, Hkv={Hkv}, d={D}, T={T}, N={N}, causal={causal}, lengths={'T / 2' if padded else 'none'}")
        modules = {}
        for fused in (False, True):
            modules[fused] = ScaledDotProductAttention(H, causal=causal, num_kv_heads=Hkv, fused_forward=fused).to(dev)
            modules[fused].set_lengths(lengths)

        def forward(fused):
            with torch.no_grad():
                return modules[fused](x)

        def both(fused):
            xg = x.detach().requires_grad_()
            (modules[fused](xg) * dout).sum().backward()
            return xg.grad

        lines.append(f"  largest difference between the modules' outputs: {(forward(True) - forward(False)).abs().max().item():.3g}")
        t_f = {fused: timed(lambda: forward(fused)) for fused in (False, True)}
        lines.append(fmt("(a) forward alone, fused_forward=False (torch formula)", t_f[False]))
        lines.append(fmt("(a) forward alone, fused_forward=True                 ", t_f[True]) + f"  torch / fused = {t_f[False][0] / t_f[True][0]:.2f}")
        kw = dict(num_kv_heads=Hkv, lengths=lengths)
        out, lse = kernels.attention_wide_forward(x, H, scale, causal, return_lse=True, **kw)
        rule = lambda: kernels.attention_wide_jac_t(dout[None], x, out, H, scale, causal, **kw)[0]   # noqa: E731
        back = lambda: kernels.attention_wide_backward(dout, x, out, lse, H, scale, causal, **kw)   # noqa: E731
        lines.append(f"  largest difference between the rule on one row and the backward kernels: {(rule() - back()).abs().max().item():.3g}")
        t_a, t_b = timed(rule), timed(back)
        lines.append(fmt("(b) backward alone, attention_wide_jac_t on one row   ", t_a))
        lines.append(fmt("(b) backward alone, attention_wide_backward           ", t_b) + f"  rule / backward = {t_a[0] / t_b[0]:.2f}")
        lines.append(f"  the range of attention_wide_backward lies wholly below that of the rule: {t_b[2] < t_a[1]}")
        lines.append(f"  largest difference between the modules' input gradients: {(both(True) - both(False)).abs().max().item():.3g}")
        t_c = {fused: timed(lambda: both(fused)) for fused in (False, True)}
        peaks = {fused: peak_extra(lambda: both(fused)) for fused in (False, True)}
        lines.append(fmt("(c) forward + backward, fused_forward=False           ", t_c[False]) + f"  peak beyond the input {peaks[False] / 2**20:.0f} MiB")
        lines.append(fmt("(c) forward + backward, fused_forward=True            ", t_c[True]) + f"  peak beyond the input {peaks[True] / 2**20:.0f} MiB"
                     f"  torch / fused = {t_c[False][0] / t_c[True][0]:.2f}")
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
