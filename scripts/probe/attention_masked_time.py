"""Time the attention rule with per-sample lengths and a sliding window on one MI355X, on the first shape of
profiles/attention_gqa_time.log: causal, H = 32, Hkv = 8, d = 128, T = 512, N = 4, V = 10.

    (a) ``kernels.attention_jac_t(..., num_kv_heads=Hkv)`` with neither lengths nor window: the entry that existed before
    (b) every length T / 2
    (c) the lengths (T, 3 T / 4, T / 2, T / 4)
    (d) ``window = 128``
    (e) the existing entry on the batch cut to ``T / 2`` positions: the live work of (b) in a grid without dead workgroups

Beside each ratio to (a) stands the ratio of the 32 x 32 tiles (query block, key block) that hold a visible pair, which this script
counts from the definition of the mask (a boolean T x T matrix per sample on the host, reduced per tile) and not from the kernel's
block ranges.  Device events, 20 calls after 3 warm-ups: median, minimum and maximum.

``--existing-only`` times (a) alone and uses no new argument: run with ``--root`` on a checkout of the parent commit it gives that
commit's kernels on the same machine; interleave it with runs on this checkout and compare the difference between the commits with
the difference between two runs of one commit.

Every invocation does its work in a child process under ``timeout``; after a child that fails or runs out of time nothing more is
started.

    python scripts/probe/attention_masked_time.py [--out FILE] [--existing-only [--root DIR] [--label TEXT]]
"""
import argparse
import os
import statistics
import subprocess
import sys

import torch

H, HKV, D, T, N, V = 32, 8, 128, 512, 4, 10
BLOCK = 32
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


def visited_tiles(lengths, window):
    """Tiles (query block, key block) with a visible pair, summed over the samples (per query head), for the causal mask."""
    t = torch.arange(T)
    dist = t[:, None] - t[None, :]
    total = 0
    for L in lengths:
        vis = (dist >= 0) & (t[:, None] < L) & (t[None, :] < L)
        if window is not None:
            vis &= dist < window
        total += int(vis.view(T // BLOCK, BLOCK, T // BLOCK, BLOCK).any(3).any(1).sum())
    return total


def fmt(name, t):
    med, lo, hi = t
    return f"  {name}: median {med * 1e3:8.3f} ms (min {lo * 1e3:8.3f}, max {hi * 1e3:8.3f})"


def run(existing_only, label):
    from vivit_amd import kernels

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    E, scale = H * D, D ** -0.5
    x = torch.randn(N, T, (H + 2 * HKV) * D, device=dev)
    M = torch.randn(V, N, T, E, device=dev)
    out = torch.randn(N, T, E, device=dev)   # (the rule takes the forward output as an operand; its values do not change the work)
    lines = [f"causal attention, H={H} query heads, Hkv={HKV} key/value heads, d={D}, T={T}, N={N}, factor rows V={V}"]
    existing = lambda: kernels.attention_jac_t(M, x, out, H, scale, True, num_kv_heads=HKV)   # noqa: E731
    t_a = timed(existing)
    lines.append(fmt(f"(a) no lengths, no window (the existing entry), {label}", t_a))
    if existing_only:
        return lines
    full = visited_tiles([T] * N, None)
    runs = (("(b) every length T/2            ", [T // 2] * N, None), ("(c) lengths T, 3T/4, T/2, T/4   ", [T, 3 * T // 4, T // 2, T // 4], None),
            ("(d) window 128                  ", None, 128))
    for name, lengths, window in runs:
        dl = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=dev)
        masked = lambda: kernels.attention_jac_t(M, x, out, H, scale, True, num_kv_heads=HKV, lengths=dl, window=window)   # noqa: E731
        t = timed(masked)
        tiles = visited_tiles(lengths or [T] * N, window)
        lines.append(fmt(name, t) + f"  time / (a) = {t[0] / t_a[0]:.3f}; visited tiles / (a) = {tiles} / {full} = {tiles / full:.3f}")
    xh, Mh, oh = x[:, :T // 2].contiguous(), M[:, :, :T // 2].contiguous(), out[:, :T // 2].contiguous()
    t = timed(lambda: kernels.attention_jac_t(Mh, xh, oh, H, scale, True, num_kv_heads=HKV))
    tiles = visited_tiles([T // 2] * N, None)
    lines.append(fmt("(e) existing entry, batch cut to T/2", t) + f"  time / (a) = {t[0] / t_a[0]:.3f}; visited tiles / (a) = {tiles} / {full} = "
                 f"{tiles / full:.3f}  (the tiles of (b); its grid has half the workgroups of (b), none of them dead)")
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
