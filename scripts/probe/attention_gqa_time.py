"""Time the grouped-query attention rule on one MI355X: ``kernels.attention_jac_t(..., num_kv_heads=Hkv)`` on the packed projection
``[N, T, (H + 2 Hkv) d]`` against what a user has without it -- K and V expanded to ``H`` heads (``repeat_interleave``, the module a
model would need in front of the multi-head attention), the multi-head kernel on ``[N, T, 3 H d]``, and dK, dV summed over each
group in torch (that module's transposed Jacobian).  One process per shape, device events, 20 calls after 3 warm-ups: median,
minimum and maximum, with the peak device memory of one call of each route above what was allocated before it.

Flops counted as profiles/attention_rule_time.log counts them (multiply-adds x 2, full T x T although the mask is causal):
10 V N H T^2 d.

``--mha-only`` times the multi-head kernel alone (no ``num_kv_heads`` argument is used): run from a checkout of an earlier commit
with this one's script, it gives that commit's kernel on the same machine.

Each shape runs in a child process of its own under ``timeout``; after a child that fails or runs out of time nothing more is
started.

    python scripts/probe/attention_gqa_time.py [--out FILE] [--mha-only [--root DIR] [--label TEXT]]
"""
import argparse
import os
import statistics
import subprocess
import sys

import torch

SHAPES = ((32, 8, 10), (32, 8, 1), (32, 1, 10), (32, 32, 10))   # (H, Hkv, V); causal, d = 128, T = 512, N = 4
D, T, N = 128, 512, 4
MFMA_F32_PEAK = 157.3e12    # flop/s, specification (fp32 matrix pipe)
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


def fmt(name, t, flops, mem):
    med, lo, hi = t
    return (f"  {name}: median {med * 1e3:8.3f} ms (min {lo * 1e3:8.3f}, max {hi * 1e3:8.3f})  {flops / med / 1e12:6.2f} Tflop/s = "
            f"{100 * flops / med / MFMA_F32_PEAK:4.1f} % of the 157.3 Tflop/s fp32-MFMA peak; peak memory above the operands "
            f"{mem / 2 ** 20:8.1f} MiB")


def run_shape(H, Hkv, V, mha_only, label=""):
    from vivit_amd import kernels

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    R, E, scale = H // Hkv, H * D, D ** -0.5
    x = torch.randn(N, T, (H + 2 * Hkv) * D, device=dev)
    M = torch.randn(V, N, T, E, device=dev)

    def expand():
        k, v = x[..., E:E + Hkv * D], x[..., E + Hkv * D:]
        rep = lambda t: t.unflatten(-1, (Hkv, D)).repeat_interleave(R, -2).flatten(-2)   # noqa: E731
        return torch.cat((x[..., :E], rep(k), rep(v)), -1)

    # the forward output, from the expanded projection (the multi-head module's formula; any route takes it as an input)
    xe = expand()
    q, k, v = xe.view(N, T, 3, H, D).permute(2, 0, 3, 1, 4)
    out = torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=True, scale=scale).transpose(1, 2).reshape(N, T, E).contiguous()
    del q, k, v
    flops = 10.0 * V * N * H * T * T * D
    KB, VC = (T + 31) // 32, 2
    lines = [f"causal attention, H={H} query heads, Hkv={Hkv} key/value heads (R={R}), d={D}, T={T}, N={N}, factor rows V={V}; "
             f"flops counted 10 V N H T^2 d = {flops / 1e9:.2f} Gflop"]
    if mha_only:
        if Hkv != H:
            return []
        mha = lambda: kernels.attention_jac_t(M, xe, out, H, scale, True)   # noqa: E731
        lines.append(fmt(f"multi-head kernel alone (no num_kv_heads), {label}", timed(mha), flops, peak_above_base(mha)))
        return lines

    def expanded():
        G = kernels.attention_jac_t(M, expand(), out, H, scale, True)
        dkv = G[..., E:].unflatten(-1, (2, Hkv, R, D)).sum(-2).flatten(-3)
        return torch.cat((G[..., :E], dkv), -1)

    native = lambda: kernels.attention_jac_t(M, x, out, H, scale, True, num_kv_heads=Hkv)   # noqa: E731
    del xe
    t_new, t_old = timed(native), timed(expanded)
    m_new, m_old = peak_above_base(native), peak_above_base(expanded)
    got, ref = native(), expanded()
    err = ((got - ref).abs().max() / ref.abs().max()).item()
    chunks = (V + VC - 1) // VC
    lines += [fmt("grouped-query kernel (num_kv_heads)              ", t_new, flops, m_new),
              fmt("expand K/V + multi-head kernel + sum over groups ", t_old, flops, m_old),
              f"  grouped / expanded time: {t_new[0] / t_old[0]:.3f}; the result is {got.numel() * 4 / 2 ** 20:.1f} MiB, the expanded qkv "
              f"{N * T * 3 * E * 4 / 2 ** 20:.1f} MiB and its factor {V * N * T * 3 * E * 4 / 2 ** 20:.1f} MiB; dK/dV workgroups "
              f"N Hkv KB x chunks = {N * Hkv * KB} x {chunks} (multi-head: {N * H * KB} x {chunks}), dQ workgroups {N * H * KB} x {chunks}; "
              f"max |difference| / max |reference|: {err:.2e}"]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--mha-only", action="store_true")
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."),
                    help="the checkout whose vivit_amd is timed")
    ap.add_argument("--label", default="this checkout", help="names the checkout in the lines of --mha-only")
    ap.add_argument("--shape", type=int, default=None, help="(child) index into SHAPES")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    if args.shape is not None:
        print("\n".join(run_shape(*SHAPES[args.shape], args.mha_only, args.label)))
        return 0
    lines, status = [], 0
    for i, (H, Hkv, _) in enumerate(SHAPES):
        if args.mha_only and H != Hkv:
            continue
        cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--root", args.root, "--shape", str(i)]
        child = subprocess.run(cmd + (["--mha-only", "--label", args.label] if args.mha_only else []), stdout=subprocess.PIPE, text=True)
        lines.append(child.stdout.rstrip("\n"))
        if child.returncode != 0:
            lines.append(f"shape {i}: exit status {child.returncode}; nothing more was started")
            status = child.returncode
            break
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a" if args.mha_only else "w") as f:
            f.write(text + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
