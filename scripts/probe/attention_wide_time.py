"""Time the attention rule at a head dimension of 256 on one MI355X: causal, H = 16, Hkv = 8, d = 256, T = 512, N = 4, V = 10.

    (a) the wide kernels (``kernels.attention_wide_jac_t``, csrc/attention_wide.hip)
    (b) what the rule did for this shape before there were wide kernels: the torch formula of the factor provider on the device
    (c) the narrow kernels at equal E: H = 32, Hkv = 16, d = 128 -- the same flops in the products dQ, dK and dV, twice the score tiles

and the peak memory beyond the operands of (a) and (b).  Device events, 20 calls after 3 warm-ups: median, minimum and maximum.

The work is done in a child process under ``timeout``; after a child that fails or runs out of time nothing more is started.

    python scripts/probe/attention_wide_time.py [--out FILE]
"""
import argparse
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from attention_scoremod_time import fmt, peak_extra, timed   # noqa: E402

H, HKV, D, N, V, T = 16, 8, 256, 4, 10, 512
STEP_SECONDS = 300


def run():
    from vivit_amd import kernels
    from vivit_amd.backend import ScaledDotProductAttention
    from vivit_amd.backend.extensions import _attention_jac_t_torch

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    E, scale = H * D, D ** -0.5
    x = torch.randn(N, T, (H + 2 * HKV) * D, device=dev)
    M = torch.randn(V, N, T, E, device=dev)
    out = torch.randn(N, T, E, device=dev)   # (the rule takes the forward output as an operand; its values do not change the work)
    lines = [f"causal, H={H} query heads, Hkv={HKV} key/value heads, d={D}, T={T}, N={N}, factor rows V={V}"]
    wide = lambda: kernels.attention_wide_jac_t(M, x, out, H, scale, True, num_kv_heads=HKV)   # noqa: E731
    t_a = timed(wide)
    lines.append(fmt("(a) the wide kernels (VC = 2, 256 threads)", t_a))
    module = ScaledDotProductAttention(H, causal=True, num_kv_heads=HKV).to(dev)
    formula = lambda: _attention_jac_t_torch(module, M, x, out)   # noqa: E731
    t_b = timed(formula, warm=2)
    lines.append(fmt("(b) the torch formula on the device", t_b) + f"  time / (a) = {t_b[0] / t_a[0]:.2f}")
    t_c = timed(lambda: kernels.attention_jac_t(M, x, out, 2 * H, (D // 2) ** -0.5, True, num_kv_heads=2 * HKV))
    lines.append(fmt(f"(c) the narrow kernels at equal E: H={2 * H}, Hkv={2 * HKV}, d={D // 2}", t_c) + f"  (a) / (c) = {t_a[0] / t_c[0]:.3f}")
    result = V * N * T * (H + 2 * HKV) * D * 4
    lines.append(f"  peak memory beyond the operands: (a) {peak_extra(wide) / 2 ** 20:.1f} MiB, (b) {peak_extra(formula) / 2 ** 20:.1f} MiB "
                 f"(the result is {result / 2 ** 20:.1f} MiB; one fp32 [V, N, H, T, T] would be {V * N * H * T * T * 4 / 2 ** 20:.1f} MiB)")
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
