"""Host checks of tests/conv_refs.py (no GPU): the two fp64 references against a literal nested-loop restatement of the
formulas of include/vivit_hip.h, the exactness precondition of every exact-family case the GPU tests use, and the planner
mirrors against the branch every case is meant for (the "expects" of the case lists, derived by hand from the planners of
csrc/factors.hip and csrc/jacobians.hip)."""
import pytest
import torch

import conv_refs as R

F64 = torch.float64

# (Cin, Cout, H, W, k, s, p, d): dilation 2; stride 3 with kernel 2 (input positions no window reads); everything asymmetric
TINY = {"dil2": (2, 2, 6, 5, 2, 1, 1, 2), "stride3-k2": (2, 3, 7, 8, 2, 3, 0, 1), "asym": (2, 2, 6, 7, (3, 2), (2, 1), (1, 2), (1, 2))}


def _tiny_operands(g, seed):
    gen = torch.Generator().manual_seed(seed)
    OH, OW = R.out_hw(*g[2:])
    M = torch.randn(2, 2, g.Cout, OH, OW, generator=gen, dtype=F64)
    x = torch.randn(2, g.Cin, g.H, g.W, generator=gen, dtype=F64)
    w = torch.randn(g.Cout, g.Cin, *g.k, generator=gen, dtype=F64)
    return M, x, w, OH, OW


@pytest.mark.parametrize("name", list(TINY))
def test_references_equal_the_loops_of_the_header(name):
    g = R.geom(*TINY[name])
    (KH, KW), (sh, sw), (ph, pw), (dh, dw) = g.k, g.s, g.p, g.d
    M, x, w, OH, OW = _tiny_operands(g, 3)
    assert OH > 1 and OW > 1
    Vw = torch.zeros(2, 2, g.Cout, g.Cin, KH, KW, dtype=F64)
    out = torch.zeros(2, 2, g.Cin, g.H, g.W, dtype=F64)
    for v in range(2):
        for n in range(2):
            for o in range(g.Cout):
                for c in range(g.Cin):
                    for a in range(KH):
                        for b in range(KW):
                            for oh in range(OH):
                                for ow in range(OW):
                                    h, ww = oh * sh - ph + a * dh, ow * sw - pw + b * dw
                                    if 0 <= h < g.H and 0 <= ww < g.W:
                                        # V[r,o,c,kh,kw] = sum M[r,o,oh,ow] x[r % N,c,h,w]
                                        Vw[v, n, o, c, a, b] += M[v, n, o, oh, ow] * x[n, c, h, ww]
                                        # out[r,ci,h,w] = sum M[r,co,oh,ow] weight[co,ci,a,b]
                                        out[v, n, c, h, ww] += M[v, n, o, oh, ow] * w[o, c, a, b]
    torch.testing.assert_close(R.weight_rule(M, x, g).reshape(Vw.shape), Vw, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(R.input_rule(M, w, g), out, rtol=1e-12, atol=1e-12)
    if name == "stride3-k2":
        assert bool((out[..., 2::3, :] == 0).all()) and bool((out[..., :, 2::3] == 0).all())   # rows / columns between the windows


def test_out_hw_is_that_of_conv2d():
    for c in R.WEIGHT_CASES + R.INPUT_CASES:
        g = c.geom
        y = torch.nn.functional.conv2d(torch.zeros(1, 1, g.H, g.W), torch.zeros(1, 1, *g.k), None, g.s, g.p, g.d)
        assert tuple(y.shape[2:]) == R.out_hw(*g[2:]), c.name


# ---- exactness precondition ------------------------------------------------------------------------------------------------
def _assert_exact(ref, mag):
    assert float(mag.max()) < 2 ** 24 and float(ref.abs().max()) < 2 ** 24
    assert bool((ref.abs() <= mag).all())
    assert torch.equal(ref, ref.round()), "not an integer"
    assert torch.equal(ref.float().double(), ref)


@pytest.mark.parametrize("name", [c.name for c in R.WEIGHT_CASES])
def test_exact_weight_case(name):
    g = R.CASES["weight"][name].geom
    M, x = R.make_case("weight", name, "exact")
    ref, _ = R.reference("weight", name, "exact")
    _assert_exact(ref, R.weight_rule_abs(M, x, g))
    assert float(ref.abs().max()) > 0


@pytest.mark.parametrize("name", [c.name for c in R.INPUT_CASES])
def test_exact_input_case(name):
    g = R.CASES["input"][name].geom
    M, w = R.make_case("input", name, "exact")
    ref, _ = R.reference("input", name, "exact")
    _assert_exact(ref, R.input_rule_abs(M, w, g))
    assert float(ref.abs().max()) > 0


def test_generic_bounds_are_positive_where_terms_exist():
    for rule, name in [("weight", "asym"), ("input", "wide-asym"), ("input", "stride3")]:
        ref, bound = R.reference(rule, name, "generic")
        assert ref.shape == bound.shape and bool((bound >= 0).all())
        assert bool((bound[ref != 0] > 0).all())


# ---- the planner mirrors pin every case to its branch -------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in R.WEIGHT_CASES])
def test_weight_plan_matches_expectation(name):
    c = R.CASES["weight"][name]
    plan = R.weight_plan(c.geom)
    assert {k: plan[k] for k in c.expects} == c.expects, plan
    if plan["route"] == "mfma":
        assert plan["lds"] <= 156 * 1024 and plan["OW"] >= 4
        assert plan["S"] == 1 or plan["nct"] * plan["S"] <= plan["threads"] // 64   # a split implies one item per wave
    off = R.weight_plan(c.geom, mfma=False)
    assert off["route"] == "scalar"


@pytest.mark.parametrize("name", [c.name for c in R.INPUT_CASES])
def test_input_plan_matches_expectation(name):
    c = R.CASES["input"][name]
    plan = R.input_plan(c.geom)
    assert {k: plan[k] for k in c.expects} == c.expects, plan
    KK = c.geom.k[0] * c.geom.k[1]
    if plan["route"] == "mfma":
        assert c.geom.Cout * KK > 1024 and plan["lds"] <= 150 * 1024
        assert plan["S"] == 1 or plan["nct"] * plan["S"] <= plan["threads"] // 64
        assert (plan["chunks"] - 1) * plan["CC"] + plan["last_CC"] == c.geom.Cout
        assert R.input_plan(c.geom, mfma=False)["route"] == "unsupported"   # what the GPU test observes in the child
    else:
        assert c.geom.Cout * KK <= 1024
        assert R.input_plan(c.geom, mfma=False) == plan


def test_case_lists_cover_the_branches_they_were_written_for():
    """The union of the cases reaches every planner branch the lists name (a case edited off its branch shows here as well)."""
    wp = {c.name: R.weight_plan(c.geom) for c in R.WEIGHT_CASES}
    mf = [p for p in wp.values() if p["route"] == "mfma"]
    assert {p["RT"] for p in mf} == {1, 2, 3, 4}
    assert {p["Lmod4"] for p in mf} == {0, 1, 2, 3}
    assert any(p["S"] > 1 and p["Lmod4"] for p in mf) and any(p["S"] > 1 and p["idle_waves"] for p in mf)
    assert {p["threads"] for p in mf} == {256, 512, 1024}
    assert {p["reason"] for p in wp.values() if p["route"] == "scalar"} == {"OW<4", "LDS", "tiny"}
    ip = {c.name: R.input_plan(c.geom) for c in R.INPUT_CASES}
    mf = [p for p in ip.values() if p["route"] == "mfma"]
    assert {p["RT"] for p in mf} == {1, 2} and {p["Qcmod4"] for p in mf} >= {0, 2, 3}
    assert any(p["chunks"] > 1 and p["S"] > 1 for p in mf) and any(p["chunks"] > 1 and p["last_CC"] != p["CC"] for p in mf)
    assert any(p["trips"] > 1 for p in mf) and any(p["Bh"] == 0 and p["Bw"] == 0 for p in mf)
    sc = [p for p in ip.values() if p["route"] == "scalar"]
    assert any(p["tiles"] and p["tiles"] > 1 and p["groups"] > 1 for p in sc) and any(p["rpw"] and p["rpw"] > 1 for p in sc)
