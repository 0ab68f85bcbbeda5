"""Time the Gram matrix of an nn.Embedding weight factor on one MI355X: the compact route (``kernels.embedding_compact`` +
``kernels.embedding_gram``, csrc/embedding.hip) against the explicit one (the factor ``[V, N, W, D]`` built with torch's
``index_add_``, then ``kernels.gram_syrk``), in one process on the same ``M`` and the same token draw: median of 20 after 3 warm-ups,
and the peak device memory of one call of each above what was allocated before it.

Token ids are Zipf-distributed (p_w ~ 1 / (w + 1)) with a fixed seed.  Multiply-adds counted: explicit n^2 W D (n = V N; the SYRK
executes about half), compact sum_w (V m_w)^2 D with m_w the number of samples that hold token w -- the kernel executes more: whole
16-sample operands per common token of a pair of sample blocks, both triangles of a diagonal block pair, class chunks of four.

The measurement runs in a child process under ``timeout``.

    python scripts/probe/embedding_gram_time.py [--out FILE]
"""
import argparse
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from vivit_amd import kernels                                        # noqa: E402

MFMA_F32_PEAK = 157.3e12    # flop/s, specification (fp32 matrix pipe)
SHAPE = (64, 128, 10, 256, 8192)   # (N, T, V, D, W)
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


def run_shape(N, T, V, D, W):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    p = 1.0 / torch.arange(1, W + 1, dtype=torch.float64)
    idx = torch.multinomial(p / p.sum(), N * T, replacement=True, generator=g).view(N, T)
    M = torch.randn(V, N, T, D, generator=g).to(dev)
    present = torch.zeros(N, W, dtype=torch.bool).scatter_(1, idx, True)
    m_w = present.sum(0).double()
    idx = idx.to(dev)
    dest = (idx + W * torch.arange(N, device=dev).unsqueeze(1)).reshape(-1)

    def explicit():
        Vt = torch.zeros((V, N * W, D), device=dev).index_add_(1, dest, M.view(V, N * T, D))
        return kernels.gram_syrk(Vt.view(V * N, W * D))

    def compact():
        return kernels.embedding_gram(*kernels.embedding_compact(M, idx))

    t_new, t_old = timed(compact), timed(explicit)
    B, ids = kernels.embedding_compact(M, idx)
    t_gram = timed(lambda: kernels.embedding_gram(B, ids))
    del B, ids
    m_new, m_old = peak_above_base(compact), peak_above_base(explicit)
    got, ref = compact(), explicit()
    err = ((got - ref).abs().max() / ref.abs().max()).item()
    n = V * N
    f_old, f_new = float(n) * n * W * D, float(((V * m_w) ** 2).sum()) * D
    lines = [f"nn.Embedding(W={W}, D={D}) on idx [N={N}, T={T}] (Zipf, seed 0: {int((m_w > 0).sum())} tokens occur, the most frequent in "
             f"{int(m_w.max())} samples), factor [V={V}, N, T, D]: Gram matrix [{n}, {n}]",
             f"  compact (embedding_compact + embedding_gram): {t_new * 1e3:9.3f} ms (embedding_gram alone {t_gram * 1e3:.3f} ms = "
             f"{100 * 2 * f_new / t_gram / MFMA_F32_PEAK:4.2f} % of the 157.3 Tflop/s fp32-MFMA peak on the multiply-adds counted); peak memory "
             f"above the operands {m_new / 2 ** 20:9.1f} MiB",
             f"  explicit (index_add_ into [V, N, W, D] + gram_syrk): {t_old * 1e3:9.3f} ms; peak memory above the operands {m_old / 2 ** 20:9.1f} MiB",
             f"  compact / explicit time: {t_new / t_old:.4f}, memory: {m_new / m_old:.5f}; multiply-adds counted: explicit n^2 W D = "
             f"{f_old / 1e9:.1f} G, compact sum_w (V m_w)^2 D = {f_new / 1e9:.3f} G (ratio {f_new / f_old:.2e}); "
             f"max |difference| / max |G|: {err:.2e}"]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help="(child) run the measurement")
    args = ap.parse_args()
    if args.child:
        print("\n".join(run_shape(*SHAPE)))
        return 0
    child = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--child"],
                           stdout=subprocess.PIPE, text=True)
    text = child.stdout.rstrip("\n")
    if child.returncode != 0:
        text += f"\nexit status {child.returncode}"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return child.returncode


if __name__ == "__main__":
    sys.exit(main())
