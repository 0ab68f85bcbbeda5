"""Time the cross-attention rule on one MI355X: H = 32, Hkv = 8, d = 128, N = 4, V = 10 (the heads of profiles/attention_gqa_time.log).

    (a) the existing self-attention entry at the shape of DESIGN.md 4.5: ``kernels.attention_jac_t``, causal, T = 512
    (b) the cost of the variant, Tq = Tk = 512: the non-causal self-attention call on a packed projection, and
        ``kernels.cross_attention_jac_t`` on the same projection split in two -- the same tiles in the same order
    (c) a decoder over a long memory, Tq = 128, Tk = 1536: both results, the query side only, the key side only
    (d) the torch formula of the factor provider on the device for (c), the only alternative a user has: time and peak memory

Device events, 20 calls after 3 warm-ups: median, minimum and maximum.

``--existing-only`` times (a) alone and uses no new name: run with ``--root`` on a checkout of the parent commit it gives that commit's
kernels on the same machine; interleave it with runs on this checkout and compare the difference between the commits with the
difference between two runs of one commit.

Every invocation does its work in a child process under ``timeout``; after a child that fails or runs out of time nothing more is
started.

    python scripts/probe/attention_cross_time.py [--out FILE] [--existing-only [--root DIR] [--label TEXT]]
"""
import argparse
import os
import statistics
import subprocess
import sys

import torch

H, HKV, D, N, V = 32, 8, 128, 4, 10
T_SELF, TQ, TK = 512, 128, 1536
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
    x = torch.randn(N, T_SELF, (H + 2 * HKV) * D, device=dev)
    M = torch.randn(V, N, T_SELF, E, device=dev)
    out = torch.randn(N, T_SELF, E, device=dev)   # (the rule takes the forward output as an operand; its values do not change the work)
    lines = [f"H={H} query heads, Hkv={HKV} key/value heads, d={D}, N={N}, factor rows V={V}"]
    t_a = timed(lambda: kernels.attention_jac_t(M, x, out, H, scale, True, num_kv_heads=HKV))
    lines.append(fmt(f"(a) self-attention, causal, T={T_SELF} (the existing entry), {label}", t_a))
    if existing_only:
        return lines
    from vivit_amd.backend import ScaledDotProductCrossAttention
    from vivit_amd.backend.extensions import _cross_attention_jac_t_torch

    t_self = timed(lambda: kernels.attention_jac_t(M, x, out, H, scale, False, num_kv_heads=HKV))
    q, kv = x[..., :E].contiguous(), x[..., E:].contiguous()
    t_cross = timed(lambda: kernels.cross_attention_jac_t(M, q, kv, out, H, scale, num_kv_heads=HKV))
    lines.append(fmt(f"(b) self-attention, not causal, T={T_SELF}                     ", t_self))
    lines.append(fmt(f"(b) cross-attention on the split projection, Tq=Tk={T_SELF}    ", t_cross) + f"  time / self = {t_cross[0] / t_self[0]:.3f}")
    del x, M, out, q, kv
    q, kv = torch.randn(N, TQ, E, device=dev), torch.randn(N, TK, 2 * HKV * D, device=dev)
    M, out = torch.randn(V, N, TQ, E, device=dev), torch.randn(N, TQ, E, device=dev)
    t_both = None
    for name, want in (("both results  ", (True, True)), ("query side only", (True, False)), ("key side only ", (False, True))):
        t = timed(lambda: kernels.cross_attention_jac_t(M, q, kv, out, H, scale, num_kv_heads=HKV, want=want))
        t_both = t_both or t
        lines.append(fmt(f"(c) cross-attention, Tq={TQ}, Tk={TK}, {name}", t) + f"  time / both = {t[0] / t_both[0]:.3f}")
    kernel_peak = peak_extra(lambda: kernels.cross_attention_jac_t(M, q, kv, out, H, scale, num_kv_heads=HKV))
    module = ScaledDotProductCrossAttention(H, num_kv_heads=HKV)
    formula = lambda: _cross_attention_jac_t_torch(module, M, q, kv, out)   # noqa: E731
    t = timed(formula, reps=20, warm=2)
    lines.append(fmt(f"(d) the torch formula on the device, Tq={TQ}, Tk={TK}, both results", t) + f"  time / (c) both = {t[0] / t_both[0]:.2f}")
    results = (V * N * TQ * E + V * N * TK * 2 * HKV * D) * 4
    lines.append(f"  peak memory beyond the operands: kernels {kernel_peak / 2 ** 20:.1f} MiB, torch formula {peak_extra(formula) / 2 ** 20:.1f} MiB "
                 f"(the two results are {results / 2 ** 20:.1f} MiB; one byte per (n, i, j) would be {N * TQ * TK / 2 ** 20:.2f} MiB)")
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
