"""Time the LayerNorm / GroupNorm rules of the factor provider on one MI355X: the HIP kernels (statistics + one visit of the factor
for the input rule and the parameter rules) against the generic autograd input rule they replace (recomputed forward +
``torch.autograd.grad(..., is_grads_batched=True)``; before the kernels existed there was no parameter rule at all), in one
process, median of 20 after 3 warm-ups.  Bytes counted: M read once, x read once, out written.

    python scripts/probe/norm_rules_time.py [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from vivit_amd.backend import extensions as ext   # noqa: E402

HBM_PEAK = 8.0e12       # B/s, specification; about 6.3e12 is what a float4 copy reaches


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


def generic_input_rule(module, M, x):
    """The fallback of ``_jac_t_mat_prod`` for a module without a kernel."""
    with torch.enable_grad():
        xi = x.detach().requires_grad_(True)
        y = module.forward(xi)
        (g,) = torch.autograd.grad(y, xi, grad_outputs=M.reshape(M.shape[0], *y.shape), is_grads_batched=True)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lines = []
    cases = [("LayerNorm(1024) on [V=10, N=128, A=64, 1024]", nn.LayerNorm(1024), (128, 64, 1024)),
             ("GroupNorm(8, 64) on [V=10, N=128, 64, 32, 32]", nn.GroupNorm(8, 64), (128, 64, 32, 32))]
    for title, module, shape in cases:
        module = module.to(dev)
        x = torch.randn(*shape, device=dev)
        module.input0 = x.clone().requires_grad_(True)     # (what the engine's forward hook leaves: the input rule is wanted)
        M = torch.randn(10, *shape, device=dev)
        nbytes = 4 * (2 * M.numel() + x.numel())

        def hip_rules():
            M.__dict__.pop("_vivit_norm_rules", None)      # a new backward pass: nothing remembered on the factor
            w = ext._param_factor(module, "weight", M, x)
            b = ext._param_factor(module, "bias", M, x)
            return ext._hip_jac_t_mat_prod(module, M, x), w, b

        t_new = timed(hip_rules)
        t_old = timed(lambda: generic_input_rule(module, M, x))
        got, ref = hip_rules()[0], generic_input_rule(module, M, x)
        err = ((got - ref).abs().max() / ref.abs().max()).item()
        lines += [title,
                  f"  HIP kernels (statistics + input rule + weight rule + bias rule): {t_new * 1e3:8.3f} ms  "
                  f"{nbytes / t_new / 1e12:5.2f} TB/s = {100 * nbytes / t_new / HBM_PEAK:4.1f} % of the 8 TB/s HBM peak",
                  f"  generic autograd input rule alone (no parameter rule existed):    {t_old * 1e3:8.3f} ms  "
                  f"{nbytes / t_old / 1e12:5.2f} TB/s",
                  f"  bytes counted (M + x + out): {nbytes / 1e9:.3f} GB; max |difference| / max |reference| of the input rule: {err:.2e}"]
        del M, x, got, ref
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
