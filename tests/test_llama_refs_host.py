"""The references and bounds of tests/llama_refs.py checked on the host: an fp32 torch emulation of every kernel of
csrc/llama_rules.hip stays inside its bound on every case the GPU tests use, and each named wrong variant falls outside on at least
one case -- bounds that a wrong kernel could pass would test nothing.  No GPU."""
import pytest
import torch

import llama_refs as R

F32 = torch.float32


def inside(got, ref, bound):
    return R.within(got, ref, bound)[0]


def rules_fp32(M, x, gamma, rstd, variant=None):
    """The rules in fp32 torch ops; ``variant`` names a deliberate mistake."""
    rs = rstd[:, None]
    h = M if gamma is None or variant == "gamma_dropped" else gamma * M
    xhat = x * rs
    if variant == "rstd_twice":
        xhat = xhat * rs
    out = h - xhat * (h * xhat).mean(2, keepdim=True)
    if variant == "layernorm_mean_kept":
        out = out - h.mean(2, keepdim=True)
    return rs * out, M * xhat


RULE_CASES = [(L, rows, V) for L in R.ROW_L for rows in R.ROWS for V in R.VS]


def rule_case(L, rows, V):
    M, x, gamma = R.make_rows(L * 31 + rows + V, V, rows, L)
    return M, x, gamma, R.fp32_stats(x)


@pytest.mark.parametrize("vec", [False, True])
def test_emulated_statistics_stay_inside(vec):
    for L in R.ROW_L:
        x = R.generic(R.gen(L), 5, L)
        got = 1.0 / torch.sqrt((x * x).mean(1) + R.RMS_EPS)
        assert inside(got, R.stats(x, R.RMS_EPS), R.stats_bound(x, R.RMS_EPS, vec)), L
        assert not inside(1.0 / torch.sqrt((x * x).mean(1)) * 1.001, R.stats(x, R.RMS_EPS), R.stats_bound(x, R.RMS_EPS, vec)), L


def test_emulated_rules_stay_inside():
    for L, rows, V in RULE_CASES:
        M, x, gamma, rstd = rule_case(L, rows, V)
        for g in (gamma, None):
            refs, mags = R.rules(M, x, g, rstd)
            got = rules_fp32(M, x, g, rstd)
            for vec in ((False, True) if L % 4 == 0 else (False,)):
                for name, a, b, c in zip(("out", "w"), got, refs, R.rules_bounds(mags, L, vec)):
                    assert inside(a, b, c), (name, L, rows, V)


@pytest.mark.parametrize("variant", ["gamma_dropped", "layernorm_mean_kept", "rstd_twice"])
def test_wrong_rules_fall_outside(variant):
    caught = 0
    for L, rows, V in RULE_CASES:
        M, x, gamma, rstd = rule_case(L, rows, V)
        refs, mags = R.rules(M, x, gamma, rstd)
        got = rules_fp32(M, x, gamma, rstd, variant)
        bounds = R.rules_bounds(mags, L, vec=False)
        caught += not (inside(got[0], refs[0], bounds[0]) and inside(got[1], refs[1], bounds[1]))
    assert caught >= len(RULE_CASES) // 2, f"{variant} passes on most cases"


def test_emulated_position_sums_stay_inside_and_a_dropped_rstd_does_not():
    for D, A, V in R.POSITION_CASES:
        g = R.gen(D + 10 * A + V)
        M, x = R.generic(g, V, 3, A, D), R.generic(g, 3, A, D)
        rstd = R.fp32_stats(x.view(3 * A, D))
        ref, bound = R.position_sums(M, x, rstd)
        assert inside((M * (x * rstd.view(3, A, 1))).sum(2), ref, bound), (D, A, V)
        assert not inside((M * x).sum(2), ref, bound), (D, A, V)


def test_rotary_emulation_and_wrong_variants():
    wrong = {"forward": 0, "v_rotated": 0}
    for d, T, H, Rr in R.ROPE_CASES:
        g = R.gen(d + 10 * T + H + Rr)
        M = R.generic(g, Rr, T, 3 * H * d)
        cos, sin = R.rope_tables(T, d)
        ref, bound = R.rope(M, cos, sin, H)
        assert inside(R.rope(M, cos, sin, H, F32)[0], ref, bound), (d, T, H, Rr)
        assert torch.equal(ref[..., 2 * H * d:], M.double()[..., 2 * H * d:])
        wrong["forward"] += not inside(R.rope_forward(M, cos, sin, H, F32), ref, bound)
        # the v third treated as a third rotated head group
        v = R.rope(torch.cat((M[..., 2 * H * d:],) * 3, -1), cos, sin, H, F32)[0][..., :H * d]
        wrong["v_rotated"] += not inside(torch.cat((ref[..., :2 * H * d].float(), v), -1), ref, bound)
        # the round trip through the module's forward formula in fp32
        y = R.rope_forward(M, cos, sin, H, F32)
        assert inside(R.rope(y, cos, sin, H, F32)[0], M.double(), R.rope_roundtrip_bound(M, H)), (d, T, H, Rr)
    # (T = 1 is position 0 alone, the identity: no variant can show there)
    n = sum(1 for c in R.ROPE_CASES if c[1] > 1)
    assert wrong["forward"] >= n and wrong["v_rotated"] >= n


def test_gate_is_exact_and_swapped_outputs_differ():
    for n in R.GATE_N:
        for V in R.VS:
            g = R.gen(n + V)
            M, a, b = R.generic(g, V, n), R.generic(g, n), R.generic(g, n)
            Ga, Gb = M * b, M * a
            # a single rounding: the fp32 product is the rounded fp64 product (which is exact: 48 bits of significand)
            assert torch.equal(Ga, (M.double() * b.double()).float()) and torch.equal(Gb, (M.double() * a.double()).float())
            assert not torch.equal(Ga, Gb)


def test_sum_depth_counts_the_kernels_tree():
    assert R.sum_depth(1, False) == 1 + 6 and R.sum_depth(1024, True) == 16 + 6 and R.sum_depth(1024, False) == 16 + 6
    assert R.sum_depth(1027, False) == 5 + 6 + 3 and R.sum_depth(4100, True) == 4 * 5 + 6 + 3


def test_guarded_buffers():
    for shift in (False, True):
        buf, view = R.guarded((3, 5), "cpu", shift)
        assert view.data_ptr() % 16 == (4 if shift else 0) and bool(torch.isnan(view).all()) and R.guards_intact(buf, view, shift)
        view.zero_()
        assert R.guards_intact(buf, view, shift)
        buf[R.GUARD_WORDS + (1 if shift else 0) + 15] = 1.0
        assert not R.guards_intact(buf, view, shift)
