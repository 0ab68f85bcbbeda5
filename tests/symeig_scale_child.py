"""The routes of the symmetric eigensolver as functions of one fp32 host matrix, shared by tests/test_symeig_scale_gpu.py and
tests/test_symeig_degenerate_gpu.py, and their child process: routes chosen by an environment variable (read once per
process) run here, ONE child per environment for a whole list of cases.

    python symeig_scale_child.py cases.json out.json

cases.json: [{"id": str, "fn": "route" | "equivariance", "route": str, "inputs": [spec, ...]}], spec = ["scaled", kind, n, rung]
or ["degenerate", kind, n, log2s] (tests/eig_edge_refs.py).  out.json: {id: {"ok": bool, "err": str, "fig": ...}}."""
import json
import sys

import numpy as np
import torch

import eig_edge_refs as R
from helpers import ROOT  # noqa: F401  (puts the repository root on sys.path)
from vivit_amd import kernels

DEV = "cuda:0"


def make_input(spec):
    what, kind, n, arg = spec
    return R.scaled_case(kind, n, arg) if what == "scaled" else R.degenerate(kind, n, arg)


def _info_zero(infos):
    for info in infos:
        assert not info.cpu().any(), f"info = {info.cpu().tolist()}"


# ---- single problems: route(A32) -> [(w, Z or None, rows or None), ...], every entry to be checked -------------------------
def route_full(A):
    """``kernels.symeig``, values only and with vectors (the size and the environment choose the reduction)."""
    G, infos = A.to(DEV), []
    w0, _ = kernels.symeig(G, eigenvectors=False, info_out=infos)
    w, Z = kernels.symeig(G, eigenvectors=True, info_out=infos)
    _info_zero(infos)
    assert torch.equal(G.cpu(), A), "input modified"
    return [(w0, None, None), (w, Z, None)]


def route_chain(A):
    with kernels.persistent_kernels(False):
        return route_full(A)


def route_rows(A):
    """Three row slices of ``symeig_rows``: each checked on its own, and all of them together."""
    from vivit_amd.distributed import row_slices

    G, n = A.to(DEV), A.shape[0]
    out, parts, w0 = [], [], None
    for lo, hi in row_slices(n, 3):
        w, Zt = kernels.symeig_rows(G, lo, hi)
        assert Zt.shape == (hi - lo, n)
        assert w0 is None or torch.equal(w, w0), "eigenvalues depend on the slice"
        w0 = w
        parts.append(Zt)
        out.append((w, Zt.T, range(lo, hi)))
    return out + [(w0, torch.cat(parts).T, None)]


def route_band(A):
    """The caller-side band reduction of the multi-GPU solver: prepare, ``sy2sb``, then the solver entered at the band."""
    n = A.shape[0]
    G = A.to(DEV).clone()
    scal = kernels.symeig_prepare_(G)
    _, tau1, band = kernels.sy2sb(G)
    w, Zt = kernels.symeig_banded_rows(band, tau1, scal, 0, n)
    return [(w, Zt.T, None)]


def _select(A, keep_of):
    plan = kernels.symeig_reduce(A.to(DEV))
    keep = keep_of(plan.evals.cpu(), A.shape[0])
    return [(plan.evals, plan.select(keep), keep)]


def keep_top(w, n):
    """The ten largest and one from the middle."""
    return sorted(set(list(range(max(n - 10, 0), n)) + [n // 2]))


def keep_many(w, n):
    """More than 256 vectors: the divide & conquer route of ``select``."""
    return list(range(n - (300 if n >= 516 else 258), n))


def keep_positive(w, n):
    """All of the cluster of positive eigenvalues."""
    return [i for i in range(n) if float(w[i]) > 0]


ROUTES = {"full": route_full, "chain": route_chain, "rows": route_rows, "band": route_band,
          "select": lambda A: _select(A, keep_top), "select_dc": lambda A: _select(A, keep_many),
          "select_cluster": lambda A: _select(A, keep_positive)}


def _same_bytes(a, b, what):
    assert a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), f"{what}: batched != single solve"


# ---- batches: every problem checked like a single one AND byte-identical to its single solve -------------------------------
def batched_values(mats):
    Gs, infos = [A.to(DEV) for A in mats], []
    W = kernels.symeigvals_batched(Gs, info_out=infos)
    _info_zero(infos)
    out = []
    for b, G in enumerate(Gs):
        _same_bytes(W[b], kernels.symeig(G, eigenvectors=False)[0], f"problem {b}")
        out.append((W[b], None, None))
    return out


def batched_select(mats):
    Gs, infos = [A.to(DEV) for A in mats], []
    n = mats[0].shape[0]
    bp = kernels.symeig_reduce_batched(Gs, info_out=infos)
    _info_zero(infos)
    keeps = [keep_top(None, n) for _ in Gs]
    Zs = bp.select(keeps)
    out = []
    for b, G in enumerate(Gs):
        single = kernels.symeig_reduce(G)
        _same_bytes(bp.evals[b], single.evals, f"problem {b} eigenvalues")
        # (the batched select back-transforms reflector by reflector, the single one in compact-WY blocks: the promise of
        # bit equality is for row b of W and for the single select run on problem b's state)
        _same_bytes(bp.plans[b].select(keeps[b]).contiguous(), single.select(keeps[b]).contiguous(), f"problem {b} eigenvectors")
        out.append((bp.evals[b], Zs[b], keeps[b]))
    return out


BATCHED = {"batched_values": batched_values, "batched_select": batched_select}


def check_route(route, mats, kinds=None):
    """Run ``route`` on the host matrices ``mats`` (one, or the problems of a batch) and ``check_eigen`` every result.
    ``kinds``: the names of the inputs; a ``dead_sample`` must also come back with an eigenvalue at zero, |w| <= 1e-5 ||A||_2
    (the residual of that pair is part of ``check_eigen``)."""
    n = mats[0].shape[0]
    small = n <= R.SMALL_N_MAX
    if route in BATCHED:
        results = BATCHED[route](mats)
        owners = mats
    else:
        results = ROUTES[route](mats[0])
        owners = [mats[0]] * len(results)
    kinds = [None] * len(owners) if kinds is None else (list(kinds) if route in BATCHED else [kinds[0]] * len(owners))
    figs = []
    for kind, A, (w, Z, rows) in zip(kinds, owners, results):
        figs.append(R.check_eigen(A, w, Z, rows, small=small))
        if kind == "dead_sample":
            assert float(w.abs().min()) <= 1e-5 * figs[-1]["norm2"], "dead sample: no eigenvalue at zero"
    return figs


def check_all(route, labelled):
    """``check_route`` for every ``(label, mats, kinds)``: all inputs run, then ONE assertion names every failing one.
    (A RuntimeError -- a device error, or info != 0 on a route that raises for it -- ends the run at once.)"""
    failed = []
    for label, mats, kinds in labelled:
        try:
            check_route(route, mats, kinds)
        except AssertionError as e:
            failed.append(f"{label}: {e}")
    assert not failed, "\n".join(failed)


def equivariance(route, n, rung):
    """``route`` on A (``dense``, rung 0) and on 2^k A on ``rung`` (sigma is 1 or an exact power of two).  Returns the figures:
    max |w_k - 2^k w_0| in ulps of ||2^k A||_2, max |Z_k - Z_0| after sign alignment, and whether both are bit-equal."""
    A0 = R.scaled("dense", n, 0)
    Ak, s = R.on_rung("dense", n, rung)
    w0, Z0, _ = ROUTES[route](A0)[-1]
    wk, Zk, _ = ROUTES[route](Ak)[-1]
    w0, wk = w0.cpu().double().numpy(), wk.cpu().double().numpy()
    Z0, Zk = Z0.cpu().double().numpy(), Zk.cpu().double().numpy()
    norm2 = float(np.abs(R.reference(Ak)[1]).max())
    sign = np.where((Z0 * Zk).sum(0) < 0, -1.0, 1.0)
    fig = {"eig_ulps": float(np.abs(wk - np.ldexp(w0, s)).max() / R.ulp32(norm2)),
           "vec": float(np.abs(Zk - Z0 * sign[None, :]).max()),
           "bit_equal": bool(np.array_equal(wk, np.ldexp(w0, s)) and np.array_equal(Zk, Z0))}
    print(f"equivariance {route} n={n} rung={rung}: {fig}")
    return fig


def main(cases_path, out_path):
    with open(cases_path) as f:
        cases = json.load(f)
    res = {}
    for case in cases:
        try:
            if case["fn"] == "equivariance":
                _, _, n, rung = case["inputs"][0]
                res[case["id"]] = {"ok": True, "fig": equivariance(case["route"], n, rung)}
            else:
                res[case["id"]] = {"ok": True, "fig": check_route(case["route"], [make_input(s) for s in case["inputs"]],
                                                                  [s[1] for s in case["inputs"]])}
        except AssertionError as e:
            res[case["id"]] = {"ok": False, "err": f"AssertionError: {e}"}
        except RuntimeError as e:
            res[case["id"]] = {"ok": False, "err": f"RuntimeError: {e}"}
            if "HIP" in str(e) or "hip" in str(e):   # a device error: nothing more runs on the GPU in this process
                break
    with open(out_path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
