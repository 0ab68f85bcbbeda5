"""Times the selective scan (csrc/selective_scan.hip) against the path a user had before it: the module's torch loop as the forward
pass and the generic rule (a recomputed forward under batched autograd) as the input rule.  Per shape, in one child process under
``timeout``: forward, rules at V = 10, forward + backward; device events, 3 warm-ups, 20 calls, median (min - max) in ms; peak memory
beyond the operands; the rules kernel's effective bandwidth from its compulsory bytes against 8 TB/s.  Writes
profiles/selective_scan_time.log (or the path given as the first argument).  The old path gets ``LIMIT`` seconds per measurement and is
reported as "did not finish" beyond them (its calls are not interrupted: the limit is checked between calls, one call at least)."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = [("mamba-130m T=256", 8, 256, 1536, 16), ("mamba-130m T=1024", 8, 1024, 1536, 16), ("D=5120 T=1024", 2, 1024, 5120, 16)]
V, WARM, CALLS, LIMIT, CHILD_LIMIT = 10, 3, 20, 20.0, 540


def measure(fn, limit=None):
    import torch
    times, start = [], time.time()
    for i in range(WARM + CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= WARM:
            times.append(a.elapsed_time(b))
        if limit is not None and time.time() - start > limit and len(times) < CALLS:
            return None if not times else (statistics.median(times), min(times), max(times), len(times))
    return statistics.median(times), min(times), max(times), len(times)


def fmt(r):
    if r is None:
        return f"did not finish a timed call in {LIMIT:.0f} s"
    return f"{r[0]:.3f} ({r[1]:.3f} - {r[2]:.3f}{'' if r[3] == CALLS else f', {r[3]} calls in {LIMIT:.0f} s'})"


def peak(fn):
    import torch
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def child(index):
    import torch
    sys.path.insert(0, ROOT)
    from vivit_amd import kernels
    from vivit_amd.backend import SelectiveScan
    from vivit_amd.backend import extensions as ext
    name, N, T, D, S = SHAPES[index]
    torch.manual_seed(0)
    mod = SelectiveScan(D, S).cuda()
    x = torch.randn(N, T, 2 * D + 2 * S, device="cuda")
    M = torch.randn(V, N, T, D, device="cuda") / T
    A_log, Dk = mod.A_log.detach(), mod.D.detach()
    print(f"{name}: N={N} T={T} D={D} S={S} V={V}; ms per call, median (min - max)")
    new_f = measure(lambda: kernels.selective_scan_forward(x, A_log, Dk))
    new_r = measure(lambda: kernels.selective_scan_rules(M, x, A_log, Dk))
    xg = x.clone().requires_grad_(True)
    new_fb = measure(lambda: mod(xg).sum().backward())
    gbytes = 4 * (M.numel() + x.numel() + V * x.numel() + V * N * D * (S + 1)) / 1e9
    print(f"  new: forward {fmt(new_f)}  rules {fmt(new_r)}  forward+backward {fmt(new_fb)}")
    print(f"  new: rules move {gbytes:.3f} GB at least: {gbytes / new_r[1] * 1e3:.0f} GB/s = {gbytes / new_r[1] * 1e3 / 80:.1f} % of 8 TB/s;"
          f" peak memory beyond the operands: forward {peak(lambda: kernels.selective_scan_forward(x, A_log, Dk)):.0f} MiB,"
          f" rules {peak(lambda: kernels.selective_scan_rules(M, x, A_log, Dk)):.0f} MiB")
    with torch.no_grad():
        old_f = measure(lambda: mod.scan_loop(x), LIMIT)
    old_fb = measure(lambda: mod.scan_loop(xg).sum().backward(), LIMIT)
    old_r = measure(lambda: ext._generic_jac_t_mat_prod(mod, M, x), LIMIT)
    print(f"  old: forward (torch loop) {fmt(old_f)}  input rule (generic) {fmt(old_r)}  forward+backward {fmt(old_fb)}")
    for what, o, n in (("forward", old_f, new_f), ("input rule vs all three rules", old_r, new_r), ("forward+backward", old_fb, new_fb)):
        if o is not None:
            print(f"  ratio {what}: {o[0] / n[0]:.1f}x")
    y_new, y_old = kernels.selective_scan_forward(x, A_log, Dk), mod.scan_loop(x).detach()
    print(f"  max |new - old| / max |old| of y: {float((y_new - y_old).abs().max() / y_old.abs().max()):.1e}")


def main():
    log = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "selective_scan_time.log")
    lines = ["selective scan (Mamba S6), one MI355X, device events, 3 warm-ups, 20 calls; new = csrc/selective_scan.hip, old = the torch loop "
             "over T and the generic rule (recomputed forward under batched autograd)"]
    for i in range(len(SHAPES)):
        p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child", str(i)],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        lines.append(p.stdout.rstrip() if p.returncode == 0 else f"{SHAPES[i][0]}: child ended with status {p.returncode}\n{p.stdout[-2000:]}")
        print(lines[-1], flush=True)
        if p.returncode != 0:
            break
    with open(log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    child(int(sys.argv[2])) if len(sys.argv) > 2 and sys.argv[1] == "--child" else main()
