"""Time the Gram matrix of an nn.Linear weight factor on a sequence input [N, T, in] on one MI355X, three ways in one process on the same
operands (vivit_amd/backend/extensions.py):

  explicit  what ViViTGGN* did before the sequence closures: ``_materialised_closures(_param_factor(...))["gram_mat"]()``, the factor
            [C, N, O, I] built by the 1 x 1 convolution rule (included in the time), then one SYRK
  route A   ``_linear_seq_weight_closures``: Gram matrices of s' and z', ``kernels.gram_seq_reduce`` (csrc/seq_linear.hip), in row slabs
  route B   the same closures: the explicit factor in chunks of the output features, each added by the SYRK

at N = 64, C = 10, (O, I) in {(3072, 768), (768, 3072)}, T in {4, 16, 64, 197}.  Per shape and route: median, minimum and maximum of
the timed calls (device events around one call; 2 warm-ups of each route, then 10 rounds, 5 where a round takes more than 0.6 s, each
round calling explicit, A, B in turn, so that drift and other work on the machine meet the three alike), the peak device memory of one
call above what was allocated before it, max |difference| / max |G| between the routes; and ``gram_seq_reduce`` alone on a block of
one class of rows (all classes where Gs is below 8 GiB), as bytes of Gs read per second of CALL time (device events around one call,
launch included: not a kernel time from a trace, and launch-bound where the call takes tens of microseconds).  From the times: the interval of
SEQ_LINEAR_KAPPA for which the planner (route A when kappa macs_A <= macs_B) never picks the slower of A and B at these shapes.

Each shape runs in a child process of its own under ``timeout``; a child that fails ends the probe.

    python scripts/probe/seq_linear_gram_time.py [--out FILE]
"""
import argparse
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from vivit_amd import kernels                                        # noqa: E402
from vivit_amd.backend import extensions as ext                      # noqa: E402

HBM_PEAK = 8.0e12           # bytes/s, specification
N, C = 64, 10
SHAPES = [(T, O, I) for (O, I) in ((3072, 768), (768, 3072)) for T in (4, 16, 64, 197)]
STEP_SECONDS = 240
MIB = 2.0 ** 20


def one_call(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    res = fn()
    t1.record()
    t1.synchronize()
    del res
    return t0.elapsed_time(t1) * 1e-3


def timed_alternating(fns, warm=2):
    """{name: sorted call times}: ``warm`` calls of each, then rounds that call every function once, in turn."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    times = {name: [] for name in fns}
    rounds = 10
    while len(times[next(iter(fns))]) < rounds:
        first = {name: one_call(fn) for name, fn in fns.items()}
        for name, t in first.items():
            times[name].append(t)
        if sum(first.values()) > 0.6:
            rounds = 5
    return {name: sorted(t) for name, t in times.items()}


def timed(fn, warm=2, reps=10):
    for _ in range(warm):
        fn()
    return sorted(one_call(fn) for _ in range(reps))


def peak_above_base(fn):
    kernels._WORKSPACES.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del res
    return peak


def forced(cl, kappa):
    def run():
        old = ext.SEQ_LINEAR_KAPPA
        ext.SEQ_LINEAR_KAPPA = kappa
        try:
            return cl["gram_mat"]()
        finally:
            ext.SEQ_LINEAR_KAPPA = old
    return run


def run_shape(T, O, I):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    s = (torch.randn(C, N, T, O, generator=g) / (N * O) ** 0.5).to(dev)
    z = torch.randn(N, T, I, generator=g).to(dev)
    n = C * N
    plan = ext._seq_linear_plan(C, N, T, O, I, kappa=1.0)
    plan_A = ext._seq_linear_plan(C, N, T, O, I, kappa=0.0)
    plan_B = ext._seq_linear_plan(C, N, T, O, I, kappa=1e30)
    module = torch.nn.Linear(1, 1)

    def explicit():
        return ext._materialised_closures(ext._param_factor(module, "weight", s, z))["gram_mat"]()

    cl = ext._linear_seq_weight_closures(s, z)
    route_A, route_B = forced(cl, 0.0), forced(cl, 1e30)
    assert plan_A["route"] == "A" and plan_B["route"] == "B"
    fns = {"explicit": explicit, "A": route_A, "B": route_B}
    times = timed_alternating(fns)
    results = {name: (statistics.median(times[name]), times[name], peak_above_base(fn)) for name, fn in fns.items()}
    G_e, G_a, G_b = explicit().view(n, n), route_A().view(n, n), route_B().view(n, n)
    scale = G_e.abs().max()
    err = {"A-explicit": ((G_a - G_e).abs().max() / scale).item(), "B-explicit": ((G_b - G_e).abs().max() / scale).item(),
           "A-B": ((G_a - G_b).abs().max() / scale).item()}
    sym = torch.equal(G_a, G_a.T) and torch.equal(G_b, G_b.T)
    del G_e, G_a, G_b

    # the kernel alone: rows of one class (all classes while Gs stays below 8 GiB) against every column
    Cr = C if 4.0 * (n * T) ** 2 <= 8 * 2.0 ** 30 else 1
    Gz = torch.randn(N * T, N * T, generator=g).to(dev)
    Gs = torch.empty(Cr * N * T, n * T, device=dev).normal_()
    out = torch.empty(Cr * N, n, device=dev)
    t_k = statistics.median(timed(lambda: kernels.gram_seq_reduce(Gz, Gs, Cr, N, C, N, T, out=out)))
    gs_bytes = 4.0 * Gs.numel()

    ratio = plan["macs_B"] / plan["macs_A"]
    bound = ext.SEQ_LINEAR_WORKSPACE_BYTES + 4 * (N * T) ** 2 + 4 * n * n
    tA, tB, tE = results["A"][0], results["B"][0], results["explicit"][0]
    lines = [f"Linear({I} -> {O}) on [N={N}, T={T}, {I}], C={C}: Gram matrix [{n}, {n}]; multiply-adds A {plan['macs_A']:.3g}, B {plan['macs_B']:.3g} "
             f"(B / A = {ratio:.3g}); route A in {len(plan_A['slabs'])} slab(s), route B in {len(plan_B['chunks'])} chunk(s); planner at kappa = "
             f"{ext.SEQ_LINEAR_KAPPA:g}: route {ext._seq_linear_plan(C, N, T, O, I)['route']}"]
    for name in ("explicit", "A", "B"):
        t, ts, peak = results[name]
        label = "explicit (factor + SYRK)" if name == "explicit" else f"route {name}"
        lines.append(f"  {label:24s}: {t * 1e3:10.3f} ms (median of {len(ts)} alternating calls, min {ts[0] * 1e3:.3f}, max {ts[-1] * 1e3:.3f}); "
                     f"peak memory above the operands {peak / MIB:9.1f} MiB")
    lines.append(f"  route A / explicit time {tA / tE:.3f}, route B / explicit {tB / tE:.3f}, A / B {tA / tB:.3f}; peak of A and B within workspace + Gz + "
                 f"one [CN, CN] matrix ({bound / MIB:.1f} MiB): A {'yes' if results['A'][2] <= bound else 'NO'}, B {'yes' if results['B'][2] <= bound else 'NO'}")
    lines.append(f"  max |difference| / max |G|: A - explicit {err['A-explicit']:.2e}, B - explicit {err['B-explicit']:.2e}, A - B {err['A-B']:.2e}; "
                 f"A and B exactly symmetric: {'yes' if sym else 'NO'}")
    lines.append(f"  gram_seq_reduce alone, rows of {Cr} class(es), Gs [{Gs.shape[0]}, {Gs.shape[1]}] = {gs_bytes / MIB:.0f} MiB: call time {t_k * 1e3:.3f} ms "
                 f"(median of 10, device events around the call) = {gs_bytes / t_k / 1e12:.3f} TB/s of Gs read ({100 * gs_bytes / t_k / HBM_PEAK:.1f} % of the 8 TB/s HBM specification"
                 f"{'; Gs fits the 256 MiB Infinity Cache, so this is not an HBM rate' if gs_bytes <= 256 * MIB else ''})")
    tsA, tsE = results["A"][1], results["explicit"][1]
    lines.append(f"KAPPA {T} {O} {I} {ratio:.6g} {tA:.6g} {tB:.6g} {tE:.6g} {tsA[0]:.6g} {tsA[-1]:.6g} {tsE[0]:.6g} {tsE[-1]:.6g}")
    return lines


def kappa_summary(rows):
    """rows: (T, O, I, macs_B / macs_A, t_A, t_B, t_explicit, min and max of A, min and max of explicit), medians of alternating
    calls.  Route A is picked when kappa <= macs_B / macs_A."""
    lo = max([r[3] for r in rows if r[4] > r[5]], default=0.0)       # A slower: kappa must exceed the ratio
    hi = min([r[3] for r in rows if r[4] <= r[5]], default=float("inf"))   # A faster: kappa must not exceed it
    out = ["", "SEQ_LINEAR_KAPPA: route A is taken when kappa * macs_A <= macs_B, i.e. kappa <= macs_B / macs_A."]
    for r in rows:
        out.append(f"  T={r[0]:3d} O={r[1]:4d} I={r[2]:4d}: macs_B / macs_A = {r[3]:8.3f}; route A {r[4] * 1e3:10.3f} ms, route B {r[5] * 1e3:10.3f} ms, "
                   f"explicit {r[6] * 1e3:10.3f} ms: {'A' if r[4] <= r[5] else 'B'} is faster")
    out.append(f"  A is slower wherever macs_B / macs_A <= {lo:.3f}; A is faster wherever macs_B / macs_A >= {hi:.3f}")
    if lo < hi:
        out.append(f"  the planner never picks the slower route at these shapes for kappa in ({lo:.3f}, {hi:.3f}]; the smallest such value, rounded up "
                   f"to three digits: {float(f'{lo * 1.0005 + 5e-4:.3g}') if lo > 0 else 0.0:g} (any positive value if A is never slower)")
    else:
        out.append("  no single kappa separates the shapes: the multiply-add model does not order them")
    wins = [r for r in rows if r[4] <= r[6]]
    out.append(f"  route A's median is at most the explicit route's at {len(wins)} of {len(rows)} shapes: " + ", ".join(f"T={r[0]} O={r[1]}" for r in wins))
    for r in rows:
        if r[3] >= ext.SEQ_LINEAR_KAPPA and r[4] > r[6]:   # the planner picks A and A's median is above explicit's
            apart = r[7] > r[10]
            out.append(f"  T={r[0]} O={r[1]} I={r[2]}: the planner picks A; A {r[4] * 1e3:.3f} ms [{r[7] * 1e3:.3f}, {r[8] * 1e3:.3f}] against explicit "
                       f"{r[6] * 1e3:.3f} ms [{r[9] * 1e3:.3f}, {r[10] * 1e3:.3f}] (median [min, max] of alternating calls): "
                       + ("every call of A is slower than every call of explicit: a loss of "
                          if apart else "the ranges overlap: within the spread, median ratio ") + f"{r[4] / r[6]:.3f}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=3, type=int, default=None, metavar=("T", "O", "I"), help="(child) measure one shape")
    args = ap.parse_args()
    if args.child:
        print("\n".join(run_shape(*args.child)))
        return 0
    text, rows, status = [], [], 0
    for T, O, I in SHAPES:
        child = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--child", str(T), str(O), str(I)],
                               stdout=subprocess.PIPE, text=True)
        for line in child.stdout.rstrip("\n").split("\n"):
            if line.startswith("KAPPA "):
                f = line.split()
                rows.append((int(f[1]), int(f[2]), int(f[3])) + tuple(float(x) for x in f[4:12]))
            else:
                text.append(line)
        print("\n".join(text[-8:]), flush=True)
        if child.returncode != 0:
            text.append(f"T={T} O={O} I={I}: exit status {child.returncode}; the probe stops here")
            status = child.returncode
            break
    if rows:
        text += kappa_summary(rows)
    print("\n".join(text[-(len(rows) + 6):]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(text) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
