"""Time the factor of a learned relative-position bias table (``kernels.attention_bias_factor``: the diagonal owner and its fold) on
one MI355X, at the shape of scripts/probe/attention_scoremod_time.py -- causal, H = 32, Hkv = 8, d = 128, T = 512, N = 4, V = 10, a
plain table ``[H, 2 T - 1]`` -- and at a T5-like shape: not causal, H = 12 heads of d = 64, T = 512, ``scale = 1``, a table ``[H, 32]``
read through ``relative_position_buckets(T, 32, 128)``; N = 4, V = 10.

    (a) the input rule with the table frozen (``kernels.attention_jac_t(..., bias=)``: the existing entry, whose instances this
        feature does not touch)
    (b) the table's factor alone, and its ratio to (a)
    (c) the torch formula of the factor provider on the device, the only alternative a user has: time and peak memory beyond the
        operands and the result

Device events, 20 calls after 3 warm-ups: median, minimum and maximum.

``--existing-only`` times (a) alone and uses no new name: run with ``--root`` on a checkout of the parent commit it gives that commit's
kernels on the same machine; interleave it with runs on this checkout and compare the difference between the commits with the
difference between two runs of one commit.

Every invocation does its work in a child process under ``timeout``; after a child that fails or runs out of time nothing more is
started.

    python scripts/probe/attention_bias_time.py [--out FILE] [--existing-only [--root DIR] [--label TEXT]]
"""
import argparse
import os
import statistics
import subprocess
import sys

import torch

N, V, T = 4, 10, 512
SHAPES = [dict(name="causal, plain table", H=32, HKV=8, D=128, causal=True, scale=None, buckets=None),
          dict(name="T5-like, not causal, scale 1, 32 buckets", H=12, HKV=12, D=64, causal=False, scale=1.0, buckets=32)]
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


def t5_buckets(max_len, num_buckets, max_distance):
    """T5's bidirectional buckets, written out here so that ``--existing-only`` needs no new name of the package."""
    import math
    r = torch.arange(-(max_len - 1), max_len)
    half = num_buckets // 2
    off, r = (r > 0).long() * half, r.abs()
    exact = half // 2
    far = exact + (torch.log(r.clamp(min=1).float() / exact) / math.log(max_distance / exact) * (half - exact)).long()
    return off + torch.where(r < exact, r, far.clamp(max=half - 1))


def run_shape(shape, existing_only, label):
    from vivit_amd import kernels

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    H, HKV, D, causal = shape["H"], shape["HKV"], shape["D"], shape["causal"]
    E, scale = H * D, shape["scale"] if shape["scale"] is not None else D ** -0.5
    x = torch.randn(N, T, (H + 2 * HKV) * D, device=dev)
    M = torch.randn(V, N, T, E, device=dev)
    out = torch.randn(N, T, E, device=dev)   # (the rules take the forward output as an operand; its values do not change the work)
    if shape["buckets"] is None:
        param, index = torch.randn(H, 2 * T - 1, device=dev), None
        table = param
    else:
        param, index = torch.randn(H, shape["buckets"], device=dev), t5_buckets(T, shape["buckets"], 128).to(dev)
        table = param[:, index].contiguous()
    lines = [f"{shape['name']}: H={H} query heads, Hkv={HKV} key/value heads, d={D}, T={T}, N={N}, factor rows V={V}"]
    t_a = timed(lambda: kernels.attention_jac_t(M, x, out, H, scale, causal, num_kv_heads=HKV, bias=table))
    lines.append(fmt(f"(a) the input rule, frozen table (the existing entry), {label}", t_a))
    if existing_only:
        return lines
    from vivit_amd.backend import ScaledDotProductAttention
    from vivit_amd.backend.extensions import _attention_bias_factor_torch

    width = param.shape[1]
    factor = lambda: kernels.attention_bias_factor(M, x, out, H, scale, causal, table, index=index, width=width if index is not None else None,   # noqa: E731
                                                   num_kv_heads=HKV)
    t_b = timed(factor)
    lines.append(fmt("(b) the table's factor alone (diagonal owner + fold, with its own lse and row dots)", t_b) + f"  time / (a) = {t_b[0] / t_a[0]:.3f}")
    kernels._WORKSPACES.clear()   # (the cached workspace is part of what the call needs: let it be allocated again, and counted)
    kernel_peak = peak_extra(factor)
    module = ScaledDotProductAttention(H, causal=causal, scale=scale, num_kv_heads=HKV, bias=param, learn_bias=True,
                                       bias_index=None if index is None else index.cpu()).to(dev)
    formula = lambda: _attention_bias_factor_torch(module, M, x, out)   # noqa: E731
    t_c = timed(formula, reps=20, warm=2)
    lines.append(fmt("(c) the torch formula on the device", t_c) + f"  time / (b) = {t_c[0] / t_b[0]:.2f}")
    result = V * N * H * width * 4
    lines.append(f"  peak memory beyond the operands and the result: kernels {(kernel_peak - result) / 2 ** 20:.1f} MiB, torch formula "
                 f"{(peak_extra(formula) - result) / 2 ** 20:.1f} MiB (the result is {result / 2 ** 20:.2f} MiB; one byte per (n, i, j) would be "
                 f"{N * T * T / 2 ** 20:.2f} MiB)")
    return lines


def run(existing_only, label):
    lines = []
    for shape in SHAPES:
        lines += run_shape(shape, existing_only, label)
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
