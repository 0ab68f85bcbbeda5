"""Child process of tests/test_eig_workspace_exact_gpu.py: every eigensolver entry of the C ABI on EXACTLY the bytes its
workspace query asks for, in the environment it was started with (the route switches are read once per process).

    python eig_workspace_exact_child.py out.json

A workspace (helpers.Guarded) is a slice of a uint8 buffer filled with 0xA5: it starts 16 bytes after a 256-byte boundary (so the
alignment slack of the query is used), is exactly as long as the query says and has at least 64 KiB of pattern before and after it.
Every case checks: status OK, info 0, the pattern around every workspace intact, and outputs byte-equal to those of the
``vivit_amd.kernels`` wrapper for the same input (which over-allocates its workspace by a quarter).  out.json: {case: "ok" | text}.
"""
import ctypes
import json
import sys

import torch

from helpers import Guarded  # (importing helpers puts the repository root on sys.path)
from vivit_amd import _lib, kernels

DEV = "cuda:0"


def same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = a.contiguous(), b.contiguous()
        assert a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), f"{what}: output {i} differs from the wrapper's"


def finish(st, info, *guards):
    torch.cuda.synchronize()
    assert st == _lib.VIVIT_OK, f"status {st}"
    assert info is None or not info.cpu().any(), f"info = {info.cpu().tolist()}"
    for g in guards:
        g.assert_intact()


def gram(n, seed):
    g = torch.Generator().manual_seed(seed)
    V = torch.randn(n, n + 40, generator=g)
    return (V @ V.T / n).to(DEV)


def f32(*shape):
    return torch.empty(shape, dtype=torch.float32, device=DEV)


def i32(count):
    return torch.zeros(count, dtype=torch.int32, device=DEV)


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr_array(tensors_or_ptrs):
    return (ctypes.c_void_p * len(tensors_or_ptrs))(*[t.data_ptr() if isinstance(t, torch.Tensor) else t for t in tensors_or_ptrs])


L = _lib.load()


def case_symeig(n, vectors):
    G = gram(n, n)
    A, w, Z, info = G.clone(), f32(n), f32(n, n) if vectors else None, i32(1)
    ws = Guarded(L.vivit_symeig_f32_workspace_bytes(n, int(vectors)))
    st = L.vivit_symeig_f32(A.data_ptr(), n, n, w.data_ptr(), Z.data_ptr() if vectors else None, n, ws.ptrs[0], ws.sizes[0],
                            info.data_ptr(), stream())
    finish(st, info, ws)
    ww, wZ = kernels.symeig(G, eigenvectors=vectors)
    same([w] + ([Z] if vectors else []), [ww] + ([wZ] if vectors else []), "symeig")


def case_rows(n, r0, r1):
    G = gram(n, n + 1)
    A, w, Zt, info = G.clone(), f32(n), f32(r1 - r0, n), i32(1)
    ws = Guarded(L.vivit_symeig_f32_workspace_bytes(n, 1))
    st = L.vivit_symeig_rows_f32(A.data_ptr(), n, n, w.data_ptr(), Zt.data_ptr(), n, r0, r1, ws.ptrs[0], ws.sizes[0], info.data_ptr(),
                                 stream())
    finish(st, info, ws)
    same([w, Zt], kernels.symeig_rows(G, r0, r1), "symeig_rows")


def case_select(n, K):
    G = gram(n, n + 2)
    keep = list(range(n - K, n))
    A, w, info = G.clone(), f32(n), i32(1)
    g = Guarded(L.vivit_symeig_reduce_f32_workspace_bytes(n), L.vivit_symeig_select_f32_workspace_bytes(n, K))
    st = L.vivit_symeig_reduce_f32(A.data_ptr(), n, n, w.data_ptr(), g.ptrs[0], g.sizes[0], info.data_ptr(), stream())
    finish(st, info, g)
    idx, Zt = torch.tensor(keep, dtype=torch.int32, device=DEV), f32(K, n)
    st = L.vivit_symeig_select_f32(A.data_ptr(), n, n, idx.data_ptr(), K, Zt.data_ptr(), n, g.ptrs[0], g.sizes[0], g.ptrs[1],
                                   g.sizes[1], info.data_ptr(), stream())
    finish(st, info, g)
    plan = kernels.symeig_reduce(G)
    same([w, Zt], [plan.evals, plan.select(keep).T], "symeig_reduce / select")


def case_values_batched(n, B):
    Gs = [gram(n, 100 + b) for b in range(B)]
    work, W, info = [G.clone() for G in Gs], f32(B, n), i32(B)
    ws = Guarded(L.vivit_symeigvals_batched_f32_workspace_bytes(n, B))
    st = L.vivit_symeigvals_batched_f32(ptr_array(work), B, n, n, W.data_ptr(), ws.ptrs[0], ws.sizes[0], info.data_ptr(), stream())
    finish(st, info, ws)
    same([W], [kernels.symeigvals_batched(Gs)], "symeigvals_batched")


def case_pairs_batched(n, Ks):
    B = len(Ks)
    Gs = [gram(n, 200 + b) for b in range(B)]
    keeps = [list(range(n - K, n)) for K in Ks]
    work, W, info = [G.clone() for G in Gs], f32(B, n), i32(B)
    each = L.vivit_symeig_reduce_f32_workspace_bytes(n)
    g = Guarded(*([each] * B), L.vivit_symeig_select_batched_f32_workspace_bytes(n, B, max(Ks)))
    states = ptr_array(g.ptrs[:B])
    st = L.vivit_symeig_reduce_batched_f32(ptr_array(work), B, n, n, W.data_ptr(), states, each, info.data_ptr(), stream())
    finish(st, info, g)
    idx = torch.tensor([k for keep in keeps for k in keep], dtype=torch.int32, device=DEV)
    Zt = f32(sum(Ks), n)
    rows = list(Zt.split(Ks))
    karr = (ctypes.c_int64 * B)(*Ks)
    st = L.vivit_symeig_select_batched_f32(ptr_array(work), B, n, n, idx.data_ptr(), karr,
                                           ptr_array([r if K else None for r, K in zip(rows, Ks)]), n, states, each, g.ptrs[B],
                                           g.sizes[B], info.data_ptr(), stream())
    finish(st, info, g)
    bp = kernels.symeig_reduce_batched(Gs)
    same([W] + rows, [bp.evals] + [Z.T for Z in bp.select(keeps)], "symeig_reduce_batched / select")


def case_sytrd_stedc(n):
    G = gram(n, n + 3)
    A, d, e, tau = G.clone(), f32(n), f32(n - 1), f32(n)
    ws = Guarded(L.vivit_sytrd_f32_workspace_bytes(n))
    st = L.vivit_sytrd_f32(A.data_ptr(), n, n, d.data_ptr(), e.data_ptr(), tau.data_ptr(), ws.ptrs[0], ws.sizes[0], stream())
    finish(st, None, ws)
    same([d, e, tau, A], kernels.sytrd(G), "sytrd")
    d2, e2, w, Z, info = d.clone(), e.clone(), f32(n), f32(n, n), i32(1)
    ws = Guarded(L.vivit_stedc_f32_workspace_bytes(n, 1))
    st = L.vivit_stedc_f32(d2.data_ptr(), e2.data_ptr(), n, w.data_ptr(), Z.data_ptr(), n, ws.ptrs[0], ws.sizes[0], info.data_ptr(),
                           stream())
    finish(st, info, ws)
    same([w, Z], kernels.stedc(d, e, eigenvectors=True), "stedc")


def case_sy2sb_panel(n, mp):
    G = gram(n, n + 4)
    nb = L.vivit_sb2st_half_bandwidth()
    A, AB, tau1 = G.clone(), f32(n, 2 * nb + 1), f32(n)
    ws = Guarded(L.vivit_sy2sb_f32_workspace_bytes(n))
    st = L.vivit_sy2sb_f32(A.data_ptr(), n, n, AB.data_ptr(), tau1.data_ptr(), ws.ptrs[0], ws.sizes[0], stream())
    finish(st, None, ws)
    same([AB, tau1, A], kernels.sy2sb(G), "sy2sb")
    pan0 = torch.randn(mp, nb, generator=torch.Generator().manual_seed(mp)).to(DEV)
    pan, Vt, tau, betas, T = pan0.clone(), f32(nb, mp), f32(nb), f32(nb), f32(nb, nb)
    ws = Guarded(L.vivit_sy2sb_panel_qr_f32_workspace_bytes(mp))
    st = L.vivit_sy2sb_panel_qr_f32(pan.data_ptr(), mp, Vt.data_ptr(), mp, tau.data_ptr(), betas.data_ptr(), T.data_ptr(), ws.ptrs[0],
                                    ws.sizes[0], stream())
    finish(st, None, ws)
    pan1 = pan0.clone()
    same([Vt, tau, betas, T, pan], list(kernels.panel_qr_(pan1)) + [pan1], "sy2sb_panel_qr")


def case_banded(n, r0, r1):
    G = gram(n, n + 5)
    A, scal = G.clone(), torch.zeros(16, dtype=torch.float32, device=DEV)
    ws = Guarded(8 * n + 256)   # (no query of its own: include/vivit_hip.h asks for 8 n + 256 bytes)
    st = L.vivit_symeig_prepare_f32(A.data_ptr(), n, n, scal.data_ptr(), ws.ptrs[0], ws.sizes[0], stream())
    finish(st, None, ws)
    B = G.clone()
    scal_w = kernels.symeig_prepare_(B)
    same([A, scal], [B, scal_w], "symeig_prepare")
    _, tau1, band = kernels.sy2sb(A)
    band2, w, Zt, info = band.clone(), f32(n), f32(r1 - r0, n), i32(1)
    ws = Guarded(L.vivit_symeig_f32_workspace_bytes(n, 1))
    st = L.vivit_symeig_banded_rows_f32(band2.data_ptr(), n, n, tau1.data_ptr(), scal.data_ptr(), w.data_ptr(), Zt.data_ptr(), n, r0,
                                        r1, ws.ptrs[0], ws.sizes[0], info.data_ptr(), stream())
    finish(st, info, ws)
    same([w, Zt], kernels.symeig_banded_rows(band, tau1, scal, r0, r1), "symeig_banded_rows")


CASES = [("symeig-200-values", lambda: case_symeig(200, False)), ("symeig-200-vectors", lambda: case_symeig(200, True)),
         ("symeig-300-values", lambda: case_symeig(300, False)), ("symeig-300-vectors", lambda: case_symeig(300, True)),
         ("rows-300-3..40", lambda: case_rows(300, 3, 40)),
         ("select-300-K11", lambda: case_select(300, 11)), ("select-300-K258", lambda: case_select(300, 258)),
         ("values-batched-200-B9", lambda: case_values_batched(200, 9)),
         ("pairs-batched-200-B9", lambda: case_pairs_batched(200, [3, 0, 11, 1, 0, 5, 2, 7, 4])),
         ("sytrd-stedc-300", lambda: case_sytrd_stedc(300)), ("sy2sb-300-panel-100", lambda: case_sy2sb_panel(300, 100)),
         ("prepare-banded-300", lambda: case_banded(300, 3, 40))]


def main(out_path):
    res = {}
    for name, fn in CASES:
        try:
            fn()
            res[name] = "ok"
        except AssertionError as e:
            res[name] = f"AssertionError: {e}"
        except RuntimeError as e:
            res[name] = f"RuntimeError: {e}"
            break   # possibly a device error: nothing more runs on the GPU in this process
        finally:
            with open(out_path, "w") as f:
                json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1])
