"""Times the Mamba-2 SSD layer (csrc/ssd.hip) against the path a user had before it: the module's torch loop as the forward pass and the
generic rule (a recomputed forward under batched autograd) as the input rule.  Per shape, in one child process under ``timeout``:
forward, rules at V = 10, forward + backward; device events, 3 warm-ups, 20 calls, median (min - max) in ms; the share of the fp32 MFMA
rate (142 TFLOP/s) from the products the kernels execute, and of 8 TB/s from their compulsory bytes.  Writes
profiles/ssd_time.log (or the path given as the first argument).  The old path gets ``LIMIT`` seconds per measurement and is reported
as "did not finish" beyond them (its calls are not interrupted: the limit is checked between calls, one call at least)."""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from selective_scan_time import CALLS, measure  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = [("mamba2-130m T=256", 8, 256, 24, 64, 128), ("mamba2-130m T=1024", 8, 1024, 24, 64, 128), ("H=80 T=1024", 2, 1024, 80, 64, 128)]
V, LIMIT, CHILD_LIMIT, MFMA_TFLOPS = 10, 10.0, 300, 142.0


def fmt(r):
    if r is None:
        return f"did not finish a timed call in {LIMIT:.0f} s"
    return f"{r[0]:.3f} ({r[1]:.3f} - {r[2]:.3f}{'' if r[3] == CALLS else f', {r[3]} calls in {LIMIT:.0f} s'})"


def child(index):
    import torch
    sys.path.insert(0, ROOT)
    from vivit_amd import kernels
    from vivit_amd.backend import SelectiveScanSSD
    from vivit_amd.backend import extensions as ext
    name, N, T, H, P, S = SHAPES[index]
    torch.manual_seed(0)
    mod = SelectiveScanSSD(H, P, S).cuda()
    x = torch.randn(N, T, H * P + H + 2 * S, device="cuda")
    M = torch.randn(V, N, T, H * P, device="cuda") / T
    params = (mod.A_log.detach(), mod.D.detach(), mod.dt_bias.detach())
    print(f"{name}: N={N} T={T} H={H} P={P} S={S} G=1 V={V}; ms per call, median (min - max)")
    new_f = measure(lambda: kernels.ssd_forward(x, *params, H, P, S))
    new_r = measure(lambda: kernels.ssd_rules(M, x, *params, H, P, S))
    xg = x.clone().requires_grad_(True)
    new_fb = measure(lambda: mod(xg).sum().backward())
    print(f"  new: forward {fmt(new_f)}  rules {fmt(new_r)}  forward+backward {fmt(new_fb)}")
    Q, R = kernels.SSD_CHUNK, kernels.SSD_CHUNK // 2   # products per chunk and (n, h), full tiles: forward 4, rules 10 and phase 1
    f_flop = 2.0 * N * H * -(-T // Q) * (Q * S * Q + Q * Q * P + 2 * Q * S * P)
    r_flop = 2.0 * N * H * -(-T // R) * (V * (R * S * R + 2 * R * P * R + 3 * R * S * P + 2 * R * R * S + R * R * R + P * R * S) + P * R * S)
    f_gb, r_gb = 4e-9 * (x.numel() + N * T * H * P), 4e-9 * (M.numel() + x.numel() + V * x.numel())
    for what, flop, gb, t in (("forward", f_flop, f_gb, new_f[1]), ("rules", r_flop, r_gb, new_r[1])):
        print(f"  new: {what} {flop / 1e9:.1f} GFLOP of products: {flop / t / 1e9:.1f} TFLOP/s = {flop / t / 1e7 / MFMA_TFLOPS:.1f} % of "
              f"{MFMA_TFLOPS:.0f} TFLOP/s; {gb:.3f} GB at least: {gb / t * 1e3:.0f} GB/s = {gb / t * 1e3 / 80:.1f} % of 8 TB/s")
    with torch.no_grad():
        old_f = measure(lambda: mod.scan_loop(x), LIMIT)
    old_fb = measure(lambda: mod.scan_loop(xg).sum().backward(), LIMIT)
    old_r = measure(lambda: ext._generic_jac_t_mat_prod(mod, M, x), LIMIT)
    print(f"  old: forward (torch loop) {fmt(old_f)}  input rule (generic) {fmt(old_r)}  forward+backward {fmt(old_fb)}")
    for what, o, n in (("forward", old_f, new_f), ("input rule vs all four rules", old_r, new_r), ("forward+backward", old_fb, new_fb)):
        if o is not None:
            print(f"  ratio {what}: {o[0] / n[0]:.1f}x" + ("" if o[0] > n[0] else "  (the kernel does NOT beat the loop here)"))
    y_new, y_old = kernels.ssd_forward(x, *params, H, P, S), mod.scan_loop(x).detach()
    print(f"  max |new - old| / max |old| of y: {float((y_new - y_old).abs().max() / y_old.abs().max()):.1e}")


def main():
    log = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ssd_time.log")
    lines = ["Mamba-2 SSD layer, one MI355X, device events, 3 warm-ups, 20 calls; new = csrc/ssd.hip, old = the torch loop over T and the "
             "generic rule (recomputed forward under batched autograd)"]
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
