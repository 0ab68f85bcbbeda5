"""fp64 references, planner mirrors and case lists for the two Conv2d rule entry points: vivit_conv2d_weight_mjp_f32
(csrc/factors.hip) and vivit_conv2d_jac_t_f32 (csrc/jacobians.hip).  TEST INFRASTRUCTURE: a plain module shared by
tests/test_conv_refs_host.py (no GPU), tests/test_conv_rules_gpu.py and its child tests/conv_rules_child.py.

The references restate the two formulas of include/vivit_hip.h in torch fp64 on the CPU (unfold + einsum for the weight
rule, autograd of F.conv2d for the input rule).  The input families are those of tests/epilogue_refs.py:

* exact: integers from {-4..4}.  Every product is an integer of magnitude <= 16 and every partial sum, in any order and on
  the matrix pipe as well as in scalar FMAs, an integer below 2^24 (tests/test_conv_refs_host.py asserts it for every
  case): the fp32 result must equal the fp64 reference BIT FOR BIT.  A dropped, duplicated or misindexed element shows.
* generic: seeded randn spread over three orders of magnitude, under the elementwise bound (n + 2) eps sum|terms| of a
  length-n sum in any order (n = OH OW for the weight rule, n = Cout KH KW for the input rule; products of two fp32
  numbers are exact in an FMA or on the matrix pipe, so the bound of epilogue_refs.sum_bound carries over).  Loose on
  purpose: it catches a precision regression, the exact family everything else.

weight_plan / input_plan restate the host planners of the two .hip files (conv2d_weight_mjp_mfma_lds; the dispatch of
vivit_conv2d_jac_t_f32 with conv2d_jac_t_mfma_plan), constants named as there.  They only label the cases and pin each to
the planner branch it is meant for: the ``expects`` of a case is asserted against its plan by the host test, and the one
route that can be observed from outside (the input rule's matrix pipe: the scalar kernels refuse those slices) by the GPU
test.  A planner change that moves a case off its branch fails the host test until the mirror and the case follow.
"""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

from epilogue_refs import EPS, exact, family, generic, misaligned  # noqa: F401  (re-exported for the tests)

F64 = torch.float64
V_SLICES, N_BATCH = 2, 3   # rows = 6: row % N matters, and 6 is no multiple of the scalar input kernel's rows per workgroup

Geom = namedtuple("Geom", "Cin Cout H W k s p d")    # k, s, p, d: (h, w) pairs
Case = namedtuple("Case", "name geom expects")


def pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def geom(Cin, Cout, H, W, k, s, p, d):
    return Geom(Cin, Cout, H, W, pair(k), pair(s), pair(p), pair(d))


def out_hw(H, W, k, s, p, d):
    """(OH, OW) of a convolution (floor mode)."""
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = pair(k), pair(s), pair(p), pair(d)
    return (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1


def cdiv(a, b):
    return -(-a // b)


# ---- references (fp64, CPU) ------------------------------------------------------------------------------------------------
def weight_rule(M, x, g):
    """V[v,n,o,(c,kh,kw)] = sum_l M[v,n,o,l] unfold(x)[n,(c,kh,kw),l]: ``M [V,N,Cout,OH,OW]``, ``x [N,Cin,H,W]`` ->
    ``[V,N,Cout,Cin KH KW]``."""
    Vd, N, Cout = M.shape[:3]
    cols = F.unfold(x.to(F64), g.k, dilation=g.d, padding=g.p, stride=g.s)
    return torch.einsum("vnol,nkl->vnok", M.to(F64).reshape(Vd, N, Cout, -1), cols)


def input_rule(M, w, g):
    """Vector-Jacobian products of x -> conv2d(x, w) for every slice: ``M [V,N,Cout,OH,OW]``, ``w [Cout,Cin,KH,KW]`` ->
    ``[V,N,Cin,H,W]``."""
    x = torch.zeros(M.shape[1], g.Cin, g.H, g.W, dtype=F64, requires_grad=True)
    y = F.conv2d(x, w.to(F64), None, g.s, g.p, g.d)
    return torch.stack([torch.autograd.grad(y, x, M[v].to(F64), retain_graph=True)[0] for v in range(M.shape[0])])


def weight_rule_abs(M, x, g):
    """sum of the absolute terms of every entry of :func:`weight_rule`."""
    return weight_rule(M.abs(), x.abs(), g)


def input_rule_abs(M, w, g):
    return input_rule(M.abs(), w.abs(), g)


def weight_bound(M, x, g):
    OH, OW = out_hw(g.H, g.W, g.k, g.s, g.p, g.d)
    return (OH * OW + 2) * EPS * weight_rule_abs(M, x, g)


def input_bound(M, w, g):
    return (g.Cout * g.k[0] * g.k[1] + 2) * EPS * input_rule_abs(M, w, g)


# ---- mirrors of the host planners ------------------------------------------------------------------------------------------
CWM_OC, CWM_U = 64, 8                 # csrc/factors.hip
CIT, CJM_IC, CJM_U = 16, 32, 8        # csrc/jacobians.hip


def _align4(v):
    return (v + 3) & ~3


def _threads(nbytes):
    return 1024 if nbytes > 80 * 1024 else (512 if nbytes > 40 * 1024 else 256)


def weight_plan(g, mfma=True, out=None):
    """conv2d_weight_mjp_mfma_lds of csrc/factors.hip (``mfma``: VIVIT_CONV_MFMA) and what the launch derives from it.
    ``out``: the (OH, OW) the entry point is given, where they are not the floor formula's (tests/conv_family_refs.py)."""
    (KH, KW), (ph, pw) = g.k, g.p
    OH, OW = out or out_hw(*g[2:])
    L, K = OH * OW, g.Cin * KH * KW
    plan = {"route": "scalar", "reason": None, "L": L, "Lmod4": L % 4, "OW": OW, "K": K, "Kmod16": K % 16, "RT": None, "S": 1,
            "threads": 256, "lds": 0, "nct": cdiv(K, 16), "trips": None, "idle_waves": None, "groups": cdiv(g.Cout, CWM_OC),
            "last_OC": g.Cout - (cdiv(g.Cout, CWM_OC) - 1) * CWM_OC}
    if not mfma or OW < 4:
        plan["reason"] = "off" if not mfma else "OW<4"
        return plan
    plane = (g.H + 2 * ph) * (g.W + 2 * pw)
    rt = cdiv(min(g.Cout, CWM_OC), 16)
    mfloats = _align4(L) * (16 * rt + 1)
    floats = _align4(g.Cin * plane) + mfloats
    if floats * 4 > 156 * 1024 or L * K < 4096:
        plan["reason"] = "LDS" if floats * 4 > 156 * 1024 else "tiny"
        return plan
    threads = _threads(floats * 4)
    nct, nw = cdiv(K, 16), threads // 64
    S = nw // nct
    while S > 1 and (S * 16 * rt * K > mfloats or (L // 4) // S < CWM_U):
        S -= 1
    S = max(S, 1)
    plan.update(route="mfma", RT=rt, S=S, threads=threads, lds=floats * 4, trips=cdiv(nct * S, nw), idle_waves=max(nw - nct * S, 0))
    return plan


def input_plan(g, mfma=True, rows=V_SLICES * N_BATCH, out=None):
    """The dispatch of vivit_conv2d_jac_t_f32 and conv2d_jac_t_mfma_plan of csrc/jacobians.hip (``mfma``: VIVIT_CONV_MFMA).
    route: "scalar", "mfma" or "unsupported".  ``out``: as for :func:`weight_plan`."""
    (KH, KW), (sh, sw), (ph, pw), (dh, dw) = g.k, g.s, g.p, g.d
    OH, OW = out or out_hw(*g[2:])
    KK, HW = KH * KW, g.H * g.W
    scalar_lds = g.Cout * KK * CIT * 4
    tiles = cdiv(HW, 256)
    plan = {"route": "unsupported", "HW": HW, "HWmod16": HW % 16, "RT": None, "S": 1, "threads": 256, "lds": 0, "CC": None,
            "chunks": None, "last_CC": None, "nct": cdiv(HW, 16), "trips": None, "Bh": None, "Bw": None, "Qcmod4": None,
            "groups": None, "last_IC": None, "rpw": None, "tiles": None}
    conv_geom = (OH - 1) * sh + (KH - 1) * dh - ph < g.H + ph and (OW - 1) * sw + (KW - 1) * dw - pw < g.W + pw
    scalar_ok = scalar_lds <= 64 * 1024 and rows * tiles <= 0x7FFFFFFF and cdiv(g.Cin, CIT) <= 65535
    if scalar_ok:
        groups = cdiv(g.Cin, CIT)
        plan.update(route="scalar", lds=scalar_lds, groups=groups, last_IC=g.Cin - (groups - 1) * CIT,
                    rpw=256 // HW if HW <= 128 else None, tiles=tiles if HW > 128 else None)
        return plan
    if not (mfma and conv_geom and cdiv(g.Cin, CJM_IC) <= 65535 and HW <= 1 << 24 and g.Cout * KK <= 1 << 24):
        return plan
    Bh = max((KH - 1) * dh - ph, 0)
    Bw = max((KW - 1) * dw - pw, 0)
    plane = (g.H + ph + Bh) * (g.W + pw + Bw)
    RT = 2 if min(g.Cin, CJM_IC) > 16 else 1
    WS = 16 * RT + 1

    def floats(cc):
        qp = _align4(cc * KK)
        return _align4(cc * plane) + qp * WS + qp

    cc = g.Cout
    while cc > 1 and floats(cc) * 4 > 150 * 1024:
        cc = (cc + 1) // 2
    if floats(cc) * 4 > 150 * 1024:
        return plan
    lds = floats(cc) * 4
    threads = _threads(lds)
    nct, nw, qp = cdiv(HW, 16), threads // 64, _align4(cc * KK)
    S = nw // nct
    while S > 1 and (nct * S * 16 * RT * 16 > qp * WS or (qp // 4) // S < CJM_U):
        S -= 1
    S = max(S, 1)
    chunks, groups = cdiv(g.Cout, cc), cdiv(g.Cin, CJM_IC)
    plan.update(route="mfma", RT=RT, S=S, threads=threads, lds=lds, CC=cc, chunks=chunks, last_CC=g.Cout - (chunks - 1) * cc,
                trips=cdiv(nct * S, nw), Bh=Bh, Bw=Bw, Qcmod4=(cc * KK) % 4, groups=groups, last_IC=g.Cin - (groups - 1) * CJM_IC)
    return plan


# ---- the cases (geometry: Cin, Cout, H, W, k, s, p, d; expects: entries of the plan the case is there for) ------------------
def _c(name, geometry, **expects):
    return Case(name, geom(*geometry), expects)


WEIGHT_CASES = [
    _c("rt3-tail", (8, 40, 11, 11, 3, 1, 0, 1), route="mfma", RT=3, L=81, Lmod4=1, S=1, trips=2),
    _c("rt2-Lmod2", (12, 20, 9, 8, 3, 1, 0, 1), route="mfma", RT=2, L=42, Lmod4=2, OW=6),
    _c("ow4", (32, 16, 6, 6, 3, 1, 0, 1), route="mfma", RT=1, OW=4, L=16, trips=5),
    _c("ow5-s2-Lmod3", (32, 16, 14, 9, 3, 2, 1, 1), route="mfma", RT=1, OW=5, L=35, Lmod4=3),
    _c("ow3-fallback", (64, 16, 5, 5, 3, 1, 0, 1), route="scalar", reason="OW<4"),
    _c("rt4-ragged-groups", (8, 150, 7, 9, 3, 1, 1, 1), route="mfma", RT=4, groups=3, last_OC=22, L=63),
    _c("two-groups", (8, 72, 10, 10, 3, 1, 1, 1), route="mfma", RT=4, groups=2, last_OC=8),
    _c("1x1-row", (64, 48, 1, 67, 1, 1, 0, 1), route="mfma", RT=3, L=67, Lmod4=3),
    _c("asym", (6, 24, 13, 17, (3, 2), (2, 1), (1, 2), (1, 2)), route="mfma", RT=2, L=133),
    _c("dil2", (8, 33, 14, 14, 3, 1, 2, 2), route="mfma", RT=3, threads=512),
    _c("stride3", (16, 16, 29, 29, 2, 3, 0, 1), route="mfma", RT=1, threads=512),
    _c("bigpad", (8, 16, 6, 6, 3, 1, 3, 1), route="mfma", RT=1),
    _c("split8", (3, 16, 32, 32, 3, 1, 1, 1), route="mfma", S=8, threads=1024),
    _c("split8-rt2", (3, 32, 32, 32, 3, 1, 1, 1), route="mfma", RT=2, S=8, lds=149040),
    _c("split2-s2-tail", (3, 16, 30, 30, 3, 2, 1, 1), route="mfma", S=2, L=225, Lmod4=1),
    _c("split7-idle-waves", (2, 16, 92, 92, 4, 6, 0, 1), route="mfma", threads=1024, nct=2, S=7, idle_waves=2, L=225),
    _c("lds-fallback", (64, 16, 32, 32, 3, 1, 1, 1), route="scalar", reason="LDS"),
    _c("tiny-4095", (7, 8, 9, 11, 3, 1, 0, 1), route="scalar", reason="tiny"),
    _c("Ktail", (5, 16, 12, 12, 3, 1, 1, 1), route="mfma", K=45, Kmod16=13),
]

INPUT_CASES = [
    _c("wide-asym", (20, 64, 9, 11, (4, 5), (2, 1), (1, 2), (1, 2)), route="mfma", RT=2, CC=32, chunks=2, last_CC=32, S=2, Bh=2, Bw=6,
       HWmod16=3),
    _c("wide-dil2", (8, 120, 10, 10, 3, 1, 2, 2), route="mfma", RT=1, CC=60, chunks=2, last_CC=60, S=2),
    _c("ragged-chunk", (8, 521, 12, 12, 3, 1, 1, 1), route="mfma", CC=66, chunks=8, last_CC=59, Qcmod4=2),
    _c("chunks+split", (8, 400, 4, 4, 3, 1, 1, 1), route="mfma", CC=100, chunks=4, last_CC=100, S=8, threads=512),
    _c("multi-trip", (40, 128, 20, 20, 3, 1, 1, 1), route="mfma", RT=2, CC=32, chunks=4, last_CC=32, S=1, trips=2, groups=2),
    _c("1x1", (4, 1030, 5, 5, 1, 1, 0, 1), route="mfma", CC=515, chunks=2, last_CC=515, S=8, Qcmod4=3),
    _c("1x1-s2", (4, 1030, 9, 9, 1, 2, 0, 1), route="mfma", CC=258, last_CC=256, S=2),
    _c("bigpad", (8, 120, 6, 6, 3, 1, 3, 1), route="mfma", Bh=0, Bw=0, S=5),
    _c("stride3", (8, 300, 10, 10, 2, 3, 0, 1), route="mfma", CC=150, chunks=2, last_CC=150),
    _c("cin33", (33, 120, 5, 5, 3, 1, 1, 1), route="mfma", RT=2, groups=2, last_IC=1, S=8),
    _c("cin17", (17, 120, 5, 7, 3, 1, 1, 1), route="mfma", RT=2, groups=1, last_IC=17, S=5),
    _c("1025-edge", (3, 1025, 4, 4, 1, 1, 0, 1), route="mfma", chunks=1, S=16, lds=139616),
    _c("1024-edge", (3, 1024, 4, 4, 1, 1, 0, 1), route="scalar", rpw=16),
    _c("scalar-tiles", (19, 8, 15, 20, 3, 1, 1, 1), route="scalar", HW=300, tiles=2, groups=2),
    _c("scalar-rpw", (5, 8, 7, 9, 3, 2, 1, 1), route="scalar", HW=63, rpw=4),
    _c("scalar-asym", (5, 7, 9, 11, (2, 3), (2, 1), (1, 2), (2, 1)), route="scalar"),
    # refused (VIVIT_E_UNSUPPORTED) while conv2d_jac_t_mfma_plan had a floor of H W Cout KH KW >= 4096 that only made sense
    # next to a scalar kernel which these slices (128 x 3 x 3 > 1024) cannot use
    _c("tiny-floor-1x3", (4, 128, 1, 3, 3, 1, 1, 1), route="mfma", RT=1, chunks=1, threads=1024, S=16),
    _c("tiny-floor-1x1", (4, 128, 1, 1, 3, 1, 1, 1), route="mfma", RT=1, chunks=1, threads=1024, S=16),
]
TINY_FLOOR = ("tiny-floor-1x3", "tiny-floor-1x1")
FAMILIES = ("exact", "generic")
CASES = {"weight": {c.name: c for c in WEIGHT_CASES}, "input": {c.name: c for c in INPUT_CASES}}


def make_case(rule, name, fam):
    """CPU fp32 operands of a case from a seeded generator: (M [V,N,Cout,OH,OW], x [N,Cin,H,W]) for the weight rule,
    (M, w [Cout,Cin,KH,KW]) for the input rule."""
    cases = WEIGHT_CASES if rule == "weight" else INPUT_CASES
    idx = [c.name for c in cases].index(name)
    g = cases[idx].geom
    gen = torch.Generator().manual_seed(10007 * idx + 101 * FAMILIES.index(fam) + (0 if rule == "weight" else 5003))
    OH, OW = out_hw(*g[2:])
    M = family(fam, gen, V_SLICES, N_BATCH, g.Cout, OH, OW)
    other = family(fam, gen, N_BATCH, g.Cin, g.H, g.W) if rule == "weight" else family(fam, gen, g.Cout, g.Cin, *g.k)
    return M, other


@functools.lru_cache(maxsize=None)
def reference(rule, name, fam):
    """(fp64 reference, elementwise bound of the generic family) of a case, computed once per process and shared by every
    test that needs it; callers must not modify the tensors."""
    g = CASES[rule][name].geom
    M, other = make_case(rule, name, fam)
    if rule == "weight":
        return weight_rule(M, other, g), weight_bound(M, other, g)
    return input_rule(M, other, g), input_bound(M, other, g)
