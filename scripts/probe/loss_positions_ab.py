"""Two builds of libvivit_hip.so in ONE process: ``vivit_ce_pos_sqrt_hessian_f32`` (csrc/loss_positions.hip, sampled, M = 1) of each on
the same device tensors, alternating -- for a change to the kernel that must not cost time, where two processes differ by more than
the change does.  Raw entry-point calls through ctypes (no provenance check: one of the two is not this tree's).

Per shape and library: median, minimum, quartiles and maximum of 40 timed calls (device events around one call; 3 warm-ups of each,
then rounds that call both, A first in even rounds and B first in odd ones), the medians of the first and second half of the rounds
(drift), and whether the two results are the same bytes.

    python scripts/probe/loss_positions_ab.py NAME_A=LIB_A NAME_B=LIB_B [--out FILE]
"""
import argparse
import ctypes
import math
import statistics

import torch

ARG = [ctypes.c_void_p] * 3 + [ctypes.c_int64] * 4 + [ctypes.c_int, ctypes.c_float, ctypes.c_void_p]


def case(libs, title, N, C, L, layout, lines, rounds=40):
    dev = torch.device("cuda:0")
    z = torch.randn(N * C * L, device=dev)
    idx = torch.randint(0, C, (N * L,), device=dev, dtype=torch.int32)
    S = {k: torch.empty(N * C * L, device=dev) for k in libs}
    scale = 1.0 / math.sqrt(N * L)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(k):
        st = libs[k].vivit_ce_pos_sqrt_hessian_f32(z.data_ptr(), idx.data_ptr(), S[k].data_ptr(), N, C, L, 1, layout, scale, stream)
        assert st == 0, st

    for k in libs:
        for _ in range(3):
            call(k)
    torch.cuda.synchronize()
    times = {k: [] for k in libs}
    names = list(libs)
    for r in range(rounds):
        for k in (names if r % 2 == 0 else names[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call(k)
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    for k in libs:
        t = sorted(times[k])
        halves = (statistics.median(times[k][:rounds // 2]), statistics.median(times[k][rounds // 2:]))
        lines.append(f"{title} {k:6s}: median {statistics.median(t):.4f} ms, min {t[0]:.4f}, quartiles {t[len(t) // 4]:.4f} / "
                     f"{t[3 * len(t) // 4]:.4f}, max {t[-1]:.4f}; medians of the first / second {rounds // 2} rounds {halves[0]:.4f} / "
                     f"{halves[1]:.4f}")
    lines.append(f"{title}: {' and '.join(names)} give the same bytes on finite logits: {torch.equal(S[names[0]], S[names[1]])}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs=2, metavar="NAME=LIB")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this probe measures on the GPU: none found")
    libs = {}
    for spec in args.libs:
        name, path = spec.split("=", 1)
        lib = ctypes.CDLL(path)
        lib.vivit_ce_pos_sqrt_hessian_f32.argtypes = ARG
        lib.vivit_ce_pos_sqrt_hessian_f32.restype = ctypes.c_int
        libs[name] = lib
    torch.manual_seed(0)
    lines = []
    case(libs, "NLC [64, 32000, 128]", 64, 32000, 128, 1, lines)
    case(libs, "NCL [16, 21, 128*128]", 16, 21, 128 * 128, 0, lines)
    case(libs, "NCL odd L [16, 21, 16383]", 16, 21, 16383, 0, lines)
    case(libs, "NLC C=1000 [64*128 rows]", 64, 1000, 128, 1, lines)
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
