"""Time the RMSNorm, gated-product and rotary rules of the factor provider on one MI355X (csrc/llama_rules.hip), each against the same
formulas through torch ops on the same device tensors -- the rule's own non-kernel path (vivit_amd/backend/extensions.py) -- and, for
the rotary embedding, against the generic autograd rule as well (a recomputed forward and ``torch.autograd.grad(...,
is_grads_batched=True)``: what a user-written module gets).

Shapes: V = 10, N = 64, T = 128; E in {768, 4096} for RMSNorm and rotary (12 heads of 64, 32 heads of 128), hidden width in {3072,
11008} for the gate.  Per shape and route: median, minimum and maximum of the timed calls (device events around one call, launches
included: a call time, not a kernel time from a trace; 2 warm-ups of each route, then 10 rounds that call every route once, in turn,
so that drift and other work on the machine meet them alike), the algorithmic bytes per second of the median against the 8 TB/s
specification, the peak device memory of one call above the operands, and max |difference| / max |reference| between the routes.

Bytes counted: RMSNorm  M + x read, the input rule written (the statistics' and the weight rule's second read of x and M are not
counted: [V, N, E] and [N T] results); gate  M read, both products written; rotary  M read, the rule written.

    python scripts/probe/llama_rules_time.py [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from vivit_amd import kernels                                        # noqa: E402
from vivit_amd.backend import RotaryEmbedding                        # noqa: E402
from vivit_amd.backend import extensions as ext                      # noqa: E402

HBM_PEAK = 8.0e12           # bytes/s, specification
V, N, T = 10, 64, 128
MIB = 2.0 ** 20


def one_call(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    res = fn()
    t1.record()
    t1.synchronize()
    del res
    return t0.elapsed_time(t1) * 1e-3


def timed_alternating(fns, warm=2, rounds=10):
    """{name: sorted call times}: ``warm`` calls of each, then rounds that call every function once, in turn."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(one_call(fn))
    return {name: sorted(t) for name, t in times.items()}


def peak_above_base(fn, reset=None):
    if reset is not None:
        reset()                                        # (results an earlier call left behind are not operands)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del res
    return peak


def first(res):
    return res[0] if isinstance(res, (tuple, list)) else res


def report(title, nbytes, fns, reference, reset=None):
    times = timed_alternating(fns)
    ref = first(fns[reference]())
    lines = [title]
    for name, fn in fns.items():
        t = times[name]
        med = statistics.median(t)
        err = ((first(fn()) - ref).abs().max() / ref.abs().max()).item()
        lines.append(f"  {name:<34s} median {med * 1e3:9.3f} ms (min {t[0] * 1e3:9.3f}, max {t[-1] * 1e3:9.3f})  "
                     f"{nbytes / med / 1e12:5.2f} TB/s = {100 * nbytes / med / HBM_PEAK:4.1f} % of 8 TB/s  "
                     f"peak memory above the operands {peak_above_base(fn, reset) / MIB:9.1f} MiB  max |diff| / max |{reference}| {err:.2e}")
    lines.append(f"  bytes counted: {nbytes / 1e9:.3f} GB")
    print("\n".join(lines), flush=True)
    return lines


def rms_case(E, dev):
    module = nn.RMSNorm(E, eps=1e-5).to(dev)
    module.weight.data.uniform_(0.5, 1.5)
    x = torch.randn(N, T, E, device=dev)
    module.input0 = x.clone().requires_grad_(True)     # (what the engine's forward hook leaves: the input rule is wanted)
    M = torch.randn(V, N, T, E, device=dev)

    def hip_rules():
        M.__dict__.pop("_vivit_rms_norm_rules", None)  # a new backward pass: nothing remembered on the factor
        w = ext._param_factor(module, "weight", M, x)
        return ext._hip_jac_t_mat_prod(module, M, x), w

    def torch_rules():
        w = (M * F.rms_norm(x, module.normalized_shape, None, module.eps).unsqueeze(0)).sum(2)
        return ext._rms_norm_jac_t_torch(module, M, x), w

    return report(f"RMSNorm({E}) on [V={V}, N={N}, T={T}, {E}]: input rule + weight rule", 4 * (2 * M.numel() + x.numel()),
                  {"HIP kernels": hip_rules, "torch formulas": torch_rules}, "torch formulas",
                  reset=lambda: M.__dict__.pop("_vivit_rms_norm_rules", None))


def gate_case(Fh, dev):
    a, b = torch.randn(N, T, Fh, device=dev), torch.randn(N, T, Fh, device=dev)
    M = torch.randn(V, N, T, Fh, device=dev)
    return report(f"gated product on [V={V}, N={N}, T={T}, {Fh}]: both factors", 4 * 3 * M.numel(),
                  {"HIP kernel": lambda: kernels.gate_jac_t(M, a, b), "torch formulas": lambda: (M * b.unsqueeze(0), M * a.unsqueeze(0))},
                  "torch formulas")


def rope_case(E, d, dev):
    module = RotaryEmbedding(E // d)
    x = torch.randn(N, T, 3 * E, device=dev)
    module(x)                                          # (the tables of the forward pass)
    M = torch.randn(V, N, T, 3 * E, device=dev)
    return report(f"rotary embedding ({E // d} heads of {d}) on [V={V}, N={N}, T={T}, {3 * E}]", 4 * 2 * M.numel(),
                  {"HIP kernel": lambda: ext._hip_jac_t_mat_prod(module, M, x), "torch formulas": lambda: ext._rope_jac_t_torch(module, M, x),
                   "generic autograd rule": lambda: ext._generic_jac_t_mat_prod(module, M, x)}, "torch formulas")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this probe measures on the GPU: none found")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lines = [f"{torch.cuda.get_device_name(0)}; call times by device events, 10 alternating rounds after 2 warm-ups of each route"]
    for case in ([lambda E=E: rms_case(E, dev) for E in (768, 4096)] + [lambda Fh=Fh: gate_case(Fh, dev) for Fh in (3072, 11008)]
                 + [lambda E=E, d=d: rope_case(E, d, dev) for E, d in ((768, 64), (4096, 128))]):
        lines += case()
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
