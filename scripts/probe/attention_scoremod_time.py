"""Time the attention rule with score modifiers on one MI355X, at the shape of scripts/probe/attention_masked_time.py: causal,
H = 32, Hkv = 8, d = 128, T = 512, N = 4, V = 10.

    (a) the existing causal entry (``kernels.attention_jac_t`` without a modifier: the plain instances)
    (b) a cap alone (c = 50, Gemma-2's), a table alone (ALiBi) and both, each as a ratio to (a)
    (c) the torch formula of the factor provider on the device for the capped and biased case, the only alternative a user has: time
        and peak memory beyond the operands

Device events, 20 calls after 3 warm-ups: median, minimum and maximum.

``--existing-only`` times (a) alone and uses no new name: run with ``--root`` on a checkout of the parent commit it gives that commit's
kernels on the same machine; interleave it with runs on this checkout and compare the difference between the commits with the
difference between two runs of one commit.

Every invocation does its work in a child process under ``timeout``; after a child that fails or runs out of time nothing more is
started.

    python scripts/probe/attention_scoremod_time.py [--out FILE] [--existing-only [--root DIR] [--label TEXT]]
"""
import argparse
import os
import statistics
import subprocess
import sys

import torch

H, HKV, D, N, V, T = 32, 8, 128, 4, 10, 512
CAP = 50.0
STEP_SECONDS = 300


def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1) * 1e-3)
    return statistics.median(times), min(times), max(times)


def fmt(name, t):
    med, lo, hi = t
    return f"  {name}: median {med * 1e3:8.3f} ms (min {lo * 1e3:8.3f}, max {hi * 1e3:8.3f})"


def peak_extra(fn):
    """Peak bytes allocated during ``fn()`` beyond what was allocated before it."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    result = fn()
    torch.cuda.synchronize()
    del result
    return torch.cuda.max_memory_allocated() - before


def run(existing_only, label):
    from vivit_amd import kernels

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    E, scale = H * D, D ** -0.5
    x = torch.randn(N, T, (H + 2 * HKV) * D, device=dev)
    M = torch.randn(V, N, T, E, device=dev)
    out = torch.randn(N, T, E, device=dev)   # (the rule takes the forward output as an operand; its values do not change the work)
    lines = [f"causal, H={H} query heads, Hkv={HKV} key/value heads, d={D}, T={T}, N={N}, factor rows V={V}"]
    t_a = timed(lambda: kernels.attention_jac_t(M, x, out, H, scale, True, num_kv_heads=HKV))
    lines.append(fmt(f"(a) no modifier (the existing entry), {label}", t_a))
    if existing_only:
        return lines
    from vivit_amd.backend import ScaledDotProductAttention, alibi_bias
    from vivit_amd.backend.extensions import _attention_jac_t_torch

    table = alibi_bias(H, T).to(dev)
    for name, kw in ((f"cap c = {CAP:g} alone     ", dict(softcap=CAP)), ("ALiBi table alone    ", dict(bias=table)),
                     ("cap and table        ", dict(softcap=CAP, bias=table))):
        t = timed(lambda: kernels.attention_jac_t(M, x, out, H, scale, True, num_kv_heads=HKV, **kw))
        lines.append(fmt(f"(b) {name}", t) + f"  time / (a) = {t[0] / t_a[0]:.3f}")
    both = lambda: kernels.attention_jac_t(M, x, out, H, scale, True, num_kv_heads=HKV, softcap=CAP, bias=table)   # noqa: E731
    t_both = timed(both)
    kernel_peak = peak_extra(both)
    module = ScaledDotProductAttention(H, causal=True, num_kv_heads=HKV, softcap=CAP, bias=table).to(dev)
    formula = lambda: _attention_jac_t_torch(module, M, x, out)   # noqa: E731
    t = timed(formula, reps=20, warm=2)
    lines.append(fmt("(c) the torch formula on the device, cap and table", t) + f"  time / (b) both = {t[0] / t_both[0]:.2f}")
    result = V * N * T * (H + 2 * HKV) * D * 4
    lines.append(f"  peak memory beyond the operands: kernels {kernel_peak / 2 ** 20:.1f} MiB, torch formula {peak_extra(formula) / 2 ** 20:.1f} MiB "
                 f"(the result is {result / 2 ** 20:.1f} MiB; one byte per (n, i, j) would be {N * T * T / 2 ** 20:.2f} MiB)")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the lines to this file")
    ap.add_argument("--existing-only", action="store_true")
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."),
                    help="the checkout whose vivit_amd is timed")
    ap.add_argument("--label", default="this commit", help="names the checkout in the line of (a)")
    ap.add_argument("--child", action="store_true", help="(internal) do the work in this process")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    if args.child:
        print("\n".join(run(args.existing_only, args.label)))
        return 0
    cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--child", "--root", args.root, "--label", args.label]
    child = subprocess.run(cmd + (["--existing-only"] if args.existing_only else []), stdout=subprocess.PIPE, text=True)
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
