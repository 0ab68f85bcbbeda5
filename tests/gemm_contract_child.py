"""Child process of tests/test_gemm_contract_gpu.py: the clean products of one GEMM route's cases, run with the environment the
parent set (the route switches VIVIT_GEMM256 / VIVIT_GEMM_BXSPLITK / VIVIT_GEMM64 / VIVIT_GEMM_TSK are read once per process);
results as a .pt file.  The parent imports this module for the same shapes and inputs.

usage: python gemm_contract_child.py ROUTE OUT.pt
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vivit_amd import kernels  # noqa: E402

DEV = torch.device("cuda:0")
LAYOUTS = ("nt", "nn", "tn")

# One shape family per public route, in the order gemm_launch (vivit_amd/csrc/gemm_f32.hip; the routes: gemm_plan.h) tries them with the default
# VIVIT_GEMM_SPLIT=6.  route -> (the switch that turns it off, or None; cases (layout, M, N, K)).
ROUTES = {
    # plan_tile256: >= 200 tiles of 256 x 256, M, N >= 512, K >= 512, one split -> bx_split_kernel + gemm256_bx_kernel with
    # the gated gemm256_kernel behind it; K = 2071: the ragged tail (7 k) goes through gemm_kernel
    "tile256": ("VIVIT_GEMM256", [(lay, 4096, 4096, k) for k in (2064, 2071) for lay in LAYOUTS]),
    # plan_bx_splitk: M, N >= 256, at most 100 tiles, K >= 16384 -> launch_bx_splitk (gated gemm256_kernel behind it)
    "splitk": ("VIVIT_GEMM_BXSPLITK", [(lay, 1000, 1300, 20480) for lay in LAYOUTS]),
    # plan_gemm64: M <= 64, N >= 2048, K >= 2048, K % 16 == 0, aligned operands -> g64_split_a_kernel + gemm64_bx_kernel
    # (NN needs M > 16: skinny_applicable takes M <= 16 first; TN needs M % 4 == 0)
    "gemm64": ("VIVIT_GEMM64", [(lay, 64, 2304, 4096) for lay in LAYOUTS] + [("nt", 1, 2048, 2048)]),
    # plan_tsk: M <= 64, N <= 1024, K >= 2048, both operands K-contiguous (NT only) -> gemm_tsk_kernel
    "tsk": ("VIVIT_GEMM_TSK", [("nt", 48, 700, 8192)]),
    # skinny_applicable: M <= 16 (vivit_gemm_nn_f32 only) -> skinny_nn_kernel
    "skinny": (None, [("nn", 8, 5000, 3000)]),
    # everything else, here lda % 4 != 0 (NT, NN) or too small for the streaming routes (TN) -> gemm_kernel
    "generic": (None, [(lay, 300, 300, 5001) for lay in LAYOUTS]),
}


# K-contiguous operands of a route stored with their leading dimension rounded up to this many floats: the 256-tile route
# needs 16-byte rows (gemm_launch's `vec`), which an unpadded lda = K = 2071 is not (that product would go to gemm_kernel)
LD_ALIGN = {"tile256": 4}


def key(case):
    lay, m, n, k = case
    return f"{lay}_{m}x{n}x{k}"


def operands(case):
    """Seeded N(0, 1) logical operands a: [M, K], b: [N, K] of a case (the product is a b^T)."""
    lay, m, n, k = case
    g = torch.Generator(device=DEV).manual_seed(m * 1000003 + n * 1009 + k)
    return torch.randn(m, k, generator=g, device=DEV), torch.randn(n, k, generator=g, device=DEV)


def _padded(x, align):
    """x (row-major) as a view into storage whose rows are rounded up to a multiple of `align` floats."""
    cols = -(-x.shape[1] // align) * align
    if cols == x.shape[1]:
        return x
    s = torch.zeros(x.shape[0], cols, device=x.device)
    s[:, :x.shape[1]] = x
    return s[:, :x.shape[1]]


def product(lay, a, b, out=None, alpha=1.0, beta=0.0, align=1):
    """alpha a b^T + beta out through the public entry point of layout `lay`, operands stored as that layout wants them
    (K-contiguous ones with rows padded to `align` floats)."""
    a_k, b_k = _padded(a, align), _padded(b, align)
    if lay == "nt":
        return kernels.gemm_nt(a_k, b_k, out=out, alpha=alpha, beta=beta)
    if lay == "nn":
        return kernels.gemm_nn(a_k, b.T.contiguous(), out=out, alpha=alpha, beta=beta)
    return kernels.gemm_tn(a.T.contiguous(), b.T.contiguous(), out=out, alpha=alpha, beta=beta)


def run(route):
    out = {}
    for case in ROUTES[route][1]:
        a, b = operands(case)
        out[key(case)] = product(case[0], a, b, align=LD_ALIGN.get(route, 1)).cpu()
    return out


if __name__ == "__main__":
    torch.save(run(sys.argv[1]), sys.argv[2])
