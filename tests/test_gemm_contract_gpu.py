"""The input-range contract of include/vivit_hip.h on every route of the public GEMMs (vivit_gemm_{nt,nn,tn}_f32), large
leading dimensions on the 64-row streaming route, and proof that each case ran the route it names.

Every public product must behave like a k-ordered fp32 fma chain for EVERY input: inf / NaN propagate as in IEEE fp32,
3.4e38 * 0.5 is finite, denormal and tiny (< 2^-100) inputs are multiplied as in fp32.  The bf16-pipe routes keep that
promise with a range gate (a flagged operand is recomputed on the fp32 matrix pipe); the fp32 routes keep it by
construction.  Shapes and routes: gemm_contract_child.ROUTES."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gemm_contract_child as child  # noqa: E402

ALPHA, BETA = 0.5, -2.0   # a fallback that applies beta twice, or writes C twice, is caught
KINDS = ("inf", "nan", "big", "den", "tiny")


def _spread(n, count):
    return [round(i * (n - 1) / (count - 1)) for i in range(count)] if count > 1 else [n // 2]


def _kpos(K, ragged_tail):
    """Columns of the special values: inside the last column chunk of the split (the one the gate must flag); with
    `ragged_tail` the inf goes to the K tail that the 256-tile route hands to gemm_kernel."""
    kmain = K // 16 * 16
    base = max(0, kmain - 1000)
    ks = {"inf": base + 100, "nan": base + 5, "big": base + 7, "den": base + 9, "tiny": base + 11}
    if ragged_tail:
        assert K > kmain
        ks["inf"] = K - 3
    return ks


def _range_cases():
    out = []
    for route, (_, cases) in child.ROUTES.items():
        for case in cases:
            lay, m, n, k = case
            for side in ("A", "B"):
                rows = m if side == "A" else n
                if rows >= len(KINDS):
                    out.append(pytest.param(route, case, side, KINDS, id=f"{route}-{child.key(case)}-{side}"))
                else:   # too few rows for all five: one case per kind
                    for kind in KINDS:
                        out.append(pytest.param(route, case, side, (kind,), id=f"{route}-{child.key(case)}-{side}-{kind}"))
    return out


@pytest.mark.parametrize("route,case,side,kinds", _range_cases())
def test_input_range_contract(route, case, side, kinds):
    """inf / NaN / 3.4e38 / 1e-39 / 1e-35 in one operand (A or B), alpha = 0.5, beta = -2 on a prefilled C: IEEE fp32 results.
    Written in the orientation of the operand X that holds the special values (its rows are rows of C for side A, columns
    for side B); Y is the partner operand."""
    lay, m, n, K = case
    dev = child.DEV
    g = torch.Generator(device=dev).manual_seed(m * 7919 + n * 31 + K + (0 if side == "A" else 1))
    nx, ny = (m, n) if side == "A" else (n, m)
    X = torch.randn(nx, K, generator=g, device=dev)
    Y = torch.randn(ny, K, generator=g, device=dev)
    C0 = torch.randn(nx, ny, generator=g, device=dev)
    ks = _kpos(K, ragged_tail=(route == "tile256" and K % 16 != 0))
    r = dict(zip(kinds, _spread(nx, len(kinds))))
    j_big = ny - 1                                  # partner row holding 1e30 opposite the denormal
    j_zero = ny // 2 if ny >= 3 else None           # partner row holding an exact 0 opposite the inf
    if "inf" in r:
        X[r["inf"], ks["inf"]] = float("inf")
        if j_zero is not None:
            Y[j_zero, ks["inf"]] = 0.0
    if "nan" in r:
        X[r["nan"], ks["nan"]] = float("nan")
    if "big" in r:
        X[r["big"]] = 0.0
        X[r["big"], ks["big"]] = 3.4e38             # bf16(3.4e38) = inf; finite in fp32
        Y[:, ks["big"]] = torch.rand(ny, generator=g, device=dev) * 1.8 - 0.9
    if "den" in r:
        X[r["den"]] = 0.0
        X[r["den"], ks["den"]] = 1e-39              # fp32 subnormal
        Y[j_big, ks["den"]] = 1e30
    if "tiny" in r:
        X[r["tiny"]] = 0.0
        X[r["tiny"], ks["tiny"]] = 1e-35            # normal, below 2^-100
        sign = torch.where(torch.rand(ny, generator=g, device=dev) < 0.5, -1.0, 1.0)
        Y[:, ks["tiny"]] = sign * (0.5 + 1.5 * torch.rand(ny, generator=g, device=dev))   # products stay normal
    for kind in ("big", "den", "tiny"):             # rows whose expected value must not drown in beta * C0
        if kind in r:
            C0[r[kind]] = 0.0

    a, b, c0 = (X, Y, C0) if side == "A" else (Y, X, C0.T.contiguous())
    C = child.product(lay, a, b, out=c0.clone(), alpha=ALPHA, beta=BETA, align=child.LD_ALIGN.get(route, 1))
    torch.cuda.synchronize()
    Cx = C if side == "A" else C.T

    # entries without a special input: finite, and as accurate as the other precision tests require
    clean = torch.ones(nx, dtype=torch.bool, device=dev)
    clean[list(r.values())] = False
    if clean.any():
        got = Cx[clean]
        assert torch.isfinite(got).all()
        Xc = X[clean].double()
        ref = ALPHA * (Xc @ Y.double().T) + BETA * C0[clean].double()
        scale = abs(ALPHA) * Xc.norm(dim=1)[:, None] * Y.double().norm(dim=1)[None, :]
        err = ((got.double() - ref).abs() / scale).max().item()
        assert err <= 5e-6, err
    if "inf" in r:   # +-inf with the sign of the partner entry; inf * 0 = NaN
        row, partner = Cx[r["inf"]], Y[:, ks["inf"]]
        zero = partner == 0
        assert row[zero].isnan().all()
        expect = torch.where(partner[~zero] > 0, float("inf"), -float("inf"))
        assert torch.equal(row[~zero], expect), (row[~zero][:8], partner[~zero][:8])
    if "nan" in r:
        assert Cx[r["nan"]].isnan().all()
    if "big" in r:   # 3.4e38 * x with |x| < 0.9 is finite in fp32 (a bf16 'hi' piece of inf would make it NaN)
        got = Cx[r["big"]].double()
        want = ALPHA * X[r["big"], ks["big"]].double() * Y[:, ks["big"]].double()
        assert torch.isfinite(got).all()
        assert ((got - want).abs() <= 1e-6 * want.abs()).all(), (got[:4], want[:4])
    if "den" in r:   # multiplied as a subnormal, not flushed: 1e-39 * 1e30 = 1e-9
        tiny = X[r["den"], ks["den"]].double().item()
        got = Cx[r["den"]].double()
        want = ALPHA * tiny * Y[:, ks["den"]].double()
        assert abs(got[j_big].item() - want[j_big].item()) <= 2e-7 * want[j_big].item(), (got[j_big].item(), want[j_big].item())
        others = torch.arange(ny, device=dev) != j_big   # subnormal products: both roundings (product, alpha) < 1.5e-45
        assert ((got - want).abs()[others] <= 2e-45).all()
    if "tiny" in r:  # exactly the fp32 product (then the exact halving)
        x = np.float32(X[r["tiny"], ks["tiny"]].item())
        y = Y[:, ks["tiny"]].cpu().numpy()
        want = (x * y).astype(np.float32) * np.float32(ALPHA)
        got = Cx[r["tiny"]].cpu().numpy()
        assert np.array_equal(got, want), np.abs(got / want - 1).max()


# ---- leading dimensions above 4.2 M floats: gemm64_bx_kernel addresses B with a 32-bit byte offset per lane, which a
# K-contiguous B wraps once 255 ldb x 4 bytes >= 2^32 (rows 239-255 of every 256-row tile would read other rows).  The
# operands are windows of NaN-filled storage: any read outside the window gives NaN or a wrong row.  A wrapped offset still
# lands inside the same allocation (off mod 2^32 < 4 GB < the B storage), so no case here reads outside its allocation.
LD = 4_500_000


@pytest.mark.parametrize("route,M,N,K", [
    ("gemm64", 64, 2048, 2048),   # plan_gemm64: M <= 64, N >= 2048, K >= 2048 (B storage ~37 GB)
    ("tsk", 64, 1024, 2048),      # plan_tsk: the next route a huge-ld NT product falls to (B storage ~18 GB)
])
def test_large_leading_dimension(route, M, N, K):
    from vivit_amd import kernels

    dev = child.DEV
    nb, na = (N - 1) * LD + K, (M - 1) * LD + K
    need = 4 * (nb + na) + 10 * 2 ** 30   # + references, output, workspace and headroom
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"needs {need / 2 ** 30:.0f} GiB of free device memory, {free / 2 ** 30:.0f} GiB free")
    g = torch.Generator(device=dev).manual_seed(N + M)
    Bs = torch.empty(nb, device=dev).fill_(float("nan"))
    Bv = Bs.as_strided((N, K), (LD, 1))
    Bv.copy_(torch.randn(N, K, generator=g, device=dev))
    As = torch.empty(na, device=dev).fill_(float("nan"))
    Av = As.as_strided((M, K), (LD, 1))
    Av.copy_(torch.randn(M, K, generator=g, device=dev))
    C = kernels.gemm_nt(Av, Bv)
    torch.cuda.synchronize()
    Ad, Bd = Av.double(), Bv.double()
    ref = Ad @ Bd.T
    assert torch.isfinite(C).all(), f"{(~torch.isfinite(C)).any(0).nonzero().flatten()[:20].tolist()} columns not finite"
    scale = Ad.norm(dim=1)[:, None] * Bd.norm(dim=1)[None, :]
    err = (C.double() - ref).abs() / scale
    assert err.max().item() <= 5e-6, f"{(err > 5e-6).any(0).nonzero().flatten()[:20].tolist()} columns wrong"


# ---- route reached: the clean products of every switchable route once more in a child process with that route's switch
# off.  Both results must match fp64, and they must NOT be bit-identical (a different kernel has a different summation
# order; with K >= 2048 random terms some entry always differs), which shows that the default ran the route named.
_ALTERNATE = {}


def _alternate(route, tmp_path_factory):
    if route not in _ALTERNATE:
        switch = child.ROUTES[route][0]
        out = str(tmp_path_factory.mktemp("route") / f"{route}.pt")
        env = dict(os.environ, **{switch: "0"})
        proc = subprocess.run([sys.executable, os.path.join(HERE, "gemm_contract_child.py"), route, out], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True, timeout=900, env=env)
        _ALTERNATE[route] = (proc.returncode, proc.stdout, torch.load(out) if proc.returncode == 0 else None)
    return _ALTERNATE[route]


@pytest.mark.parametrize("route,case", [pytest.param(r, c, id=f"{r}-{child.key(c)}")
                                        for r, (sw, cs) in child.ROUTES.items() if sw for c in cs])
def test_route_reached(route, case, tmp_path_factory):
    status, log, alt = _alternate(route, tmp_path_factory)
    assert status == 0, log[-3000:]
    a, b = child.operands(case)
    default = child.product(case[0], a, b, align=child.LD_ALIGN.get(route, 1)).cpu()
    other = alt[child.key(case)]
    ad, bd = a.double(), b.double()
    ref = (ad @ bd.T).cpu()
    scale = (ad.norm(dim=1)[:, None] * bd.norm(dim=1)[None, :]).cpu()
    for name, c in (("default", default), (child.ROUTES[route][0] + "=0", other)):
        err = ((c.double() - ref).abs() / scale).max().item()
        assert err <= 5e-6, (name, err)
    assert not torch.equal(default, other), f"{child.ROUTES[route][0]}=0 gave bit-identical results: the route was not taken"
