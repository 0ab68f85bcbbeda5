"""Time the attention rule of the factor provider on one MI355X: the HIP kernels (row log-sum-exp, row dots, the key-block owner and
the query-block owner: ``kernels.attention_jac_t``) against the generic autograd rule they replace (recomputed forward +
``torch.autograd.grad(..., is_grads_batched=True)``: ``_generic_jac_t_mat_prod``, what ``_jac_t_mat_prod`` calls for a module
without a kernel), in one process, median of 20 after 3 warm-ups, with the peak device memory of one call of each above what was
allocated before it.

Flops counted (multiply-adds x 2, per factor row, sample and head, full T x T): the five products S, dP, dV, dK, dQ = 10 T^2 d; the
kernels execute more (S once more in the second owner, both per chunk of factor rows, and the padding to tiles).

Each shape runs in a child process of its own under ``timeout`` (both rules of a shape in the same process); after a child that
fails or runs out of time nothing more is started.

    python scripts/probe/attention_rule_time.py [--out FILE]
"""
import argparse
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from vivit_amd import kernels                                        # noqa: E402
from vivit_amd.backend import ScaledDotProductAttention             # noqa: E402
from vivit_amd.backend.extensions import _generic_jac_t_mat_prod    # noqa: E402

MFMA_F32_PEAK = 157.3e12    # flop/s, specification (fp32 matrix pipe)
SHAPES = ((10, 64, 197, 384, 6), (1, 64, 197, 384, 6))   # (V, N, T, E, H)
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
    return statistics.median(times)


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


def run_shape(V, N, T, E, H):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lines = []
    d = E // H
    module = ScaledDotProductAttention(H)
    x = torch.randn(N, T, 3 * E, device=dev)
    with torch.no_grad():
        out = module(x)
    M = torch.randn(V, N, T, E, device=dev)
    scale = module.scale_for(d)
    native = lambda: kernels.attention_jac_t(M, x, out, H, scale, False)   # noqa: E731
    generic = lambda: _generic_jac_t_mat_prod(module, M, x)                # noqa: E731
    t_new, t_old = timed(native), timed(generic)
    m_new, m_old = peak_above_base(native), peak_above_base(generic)
    got, ref = native(), generic()
    err = ((got - ref).abs().max() / ref.abs().max()).item()
    flops = 10.0 * V * N * H * T * T * d
    nbytes = 4 * (M.numel() + x.numel() + out.numel() + got.numel())
    lines += [f"ScaledDotProductAttention(H={H}) on qkv [N={N}, T={T}, 3 E={3 * E}], factor [V={V}, N, T, E] (d = {d})",
              f"  HIP kernels (lse + row dots + dK/dV owner + dQ owner): {t_new * 1e3:9.3f} ms  {flops / t_new / 1e12:6.2f} Tflop/s = "
              f"{100 * flops / t_new / MFMA_F32_PEAK:4.1f} % of the 157.3 Tflop/s fp32-MFMA peak; peak memory above the operands "
              f"{m_new / 2 ** 20:9.1f} MiB (the result is {got.numel() * 4 / 2 ** 20:.1f} MiB)",
              f"  generic autograd rule (recomputed forward, batched grad): {t_old * 1e3:9.3f} ms  {flops / t_old / 1e12:6.2f} Tflop/s; "
              f"peak memory above the operands {m_old / 2 ** 20:9.1f} MiB",
              f"  native / generic time: {t_new / t_old:.3f}; flops counted 10 V N H T^2 d = {flops / 1e9:.2f} Gflop; compulsory bytes "
              f"(M + qkv + out + G) {nbytes / 1e9:.3f} GB; max |difference| / max |reference|: {err:.2e}"]
    del M, x, out, got, ref
    torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", type=int, default=None, help="(child) index into SHAPES")
    args = ap.parse_args()
    if args.shape is not None:
        print("\n".join(run_shape(*SHAPES[args.shape])))
        return 0
    lines, status = [], 0
    for i in range(len(SHAPES)):
        child = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--shape", str(i)],
                               stdout=subprocess.PIPE, text=True)
        lines.append(child.stdout.rstrip("\n"))
        if child.returncode != 0:
            lines.append(f"shape {i}: exit status {child.returncode}; nothing more was started")
            status = child.returncode
            break
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
