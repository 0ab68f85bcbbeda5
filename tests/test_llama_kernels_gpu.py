"""The RMSNorm, gated-product and rotary kernels (csrc/llama_rules.hip) at their edge shapes through the wrappers of
vivit_amd.kernels, against fp64 references under the derived bounds of tests/llama_refs.py (the gate: bit for bit).

Outputs are views between guard words, pre-filled with NaN: every element must be written and no word around them.  Row lengths:
1, 3, 64, 255 | 256 (scalar | 16-byte body), 1024 | 1027 (the last row a wavefront holds | the workgroup route, ragged) and 4100
(multi-trip); 1, 5 and 7 rows are no multiples of the four rows per workgroup."""
import pytest
import torch

import llama_refs as R
from vivit_amd import _lib, kernels
from vivit_amd.backend import RotaryEmbedding

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def check(got, ref, bound, what):
    ok, msg = R.within(got.cpu(), ref, bound)
    assert ok, f"{what}: {msg}"


def dev(t, shift=False):
    return None if t is None else (R.misaligned(t.to(DEV)) if shift else t.to(DEV))


def run_rules(M, x, gamma, rstd, want=(True, True), shift=()):
    """The rules into guarded buffers; ``shift``: names of the operands that sit 4 bytes off 16-byte alignment."""
    bufs = [R.guarded(M.shape, DEV, name in shift) if w else (None, None) for w, name in zip(want, ("out", "w"))]
    out, w = kernels.rms_norm_rules(dev(M, "M" in shift), dev(x, "x" in shift), dev(gamma, "gamma" in shift), dev(rstd), want,
                                    out=bufs[0][1], w=bufs[1][1])
    for (buf, view), got, name in zip(bufs, (out, w), ("out", "w")):
        assert (got is None) if view is None else (got is view and R.guards_intact(buf, view, name in shift)), name
        assert got is None or not bool(torch.isnan(got).any()), f"{name}: elements left unwritten"
    return out, w


# ---- RMSNorm ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [False, True], ids=["aligned", "offset4"])
@pytest.mark.parametrize("L", R.ROW_L)
def test_rms_norm_stats(L, shift):
    for rows in R.ROWS:
        x = R.generic(R.gen(L + rows), rows, L)
        rstd = kernels.rms_norm_stats(dev(x, shift), rows, R.RMS_EPS)
        check(rstd, R.stats(x, R.RMS_EPS), R.stats_bound(x, R.RMS_EPS, vec=L % 4 == 0 and not shift), f"rstd L={L} rows={rows}")
        assert torch.equal(rstd, kernels.rms_norm_stats(dev(x, shift), rows, R.RMS_EPS))
    # a row of zeros: rstd = 1 / sqrt(eps); and eps = 0 on ordinary rows
    z = kernels.rms_norm_stats(torch.zeros(2, L, device=DEV), 2, 0.25)
    assert torch.equal(z.cpu(), torch.full((2,), 2.0))
    check(kernels.rms_norm_stats(dev(x, shift), rows, 0.0), R.stats(x, 0.0), R.stats_bound(x, 0.0, vec=L % 4 == 0 and not shift), "eps = 0")


@pytest.mark.parametrize("V", R.VS)
@pytest.mark.parametrize("L", R.ROW_L)
def test_rms_norm_rules(L, V):
    for rows in R.ROWS:
        M, x, gamma = R.make_rows(L * 31 + rows + V, V, rows, L)
        rstd = R.fp32_stats(x)
        for g in (gamma, None):
            refs, mags = R.rules(M, x, g, rstd)
            got = run_rules(M, x, g, rstd)
            for name, g_, r_, b_ in zip(("out", "w"), got, refs, R.rules_bounds(mags, L, vec=L % 4 == 0)):
                check(g_, r_, b_, f"{name} L={L} rows={rows} V={V} gamma={g is not None}")


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("L", [3, 256, 1024, 1027, 4100])
def test_rms_norm_rules_null_outputs(L, skip):
    """out or w NULL: the other one bit for bit that of the full call."""
    M, x, gamma = R.make_rows(L, 2, 5, L)
    rstd = R.fp32_stats(x)
    full = run_rules(M, x, gamma, rstd)
    part = run_rules(M, x, gamma, rstd, want=tuple(i != skip for i in range(2)))
    assert part[skip] is None and torch.equal(part[1 - skip], full[1 - skip])


@pytest.mark.parametrize("which", ["M", "x", "gamma", "out", "w"])
@pytest.mark.parametrize("L", [256, 4100])
def test_rms_norm_rules_offset_pointer(L, which):
    """One operand four bytes off a 16-byte boundary: the scalar body."""
    M, x, gamma = R.make_rows(L + len(which), 2, 5, L)
    rstd = R.fp32_stats(x)
    refs, mags = R.rules(M, x, gamma, rstd)
    got = run_rules(M, x, gamma, rstd, shift=(which,))
    for name, g_, r_, b_ in zip(("out", "w"), got, refs, R.rules_bounds(mags, L, vec=False)):
        check(g_, r_, b_, f"{name}, {which} offset")


def test_rms_norm_many_rows():
    """70 000 rows of three elements: beyond 65 535 in every grid dimension a launch could have used for them."""
    rows, L = 70000, 3
    M, x, gamma = R.make_rows(11, 1, rows, L)
    rstd = R.fp32_stats(x)
    refs, mags = R.rules(M, x, gamma, rstd)
    for name, g_, r_, b_ in zip(("out", "w"), run_rules(M, x, gamma, rstd), refs, R.rules_bounds(mags, L, vec=False)):
        check(g_, r_, b_, name)
    check(kernels.rms_norm_stats(x.to(DEV), rows, R.RMS_EPS), R.stats(x, R.RMS_EPS), R.stats_bound(x, R.RMS_EPS, vec=False), "rstd")


@pytest.mark.parametrize("L", [64, 255, 256, 1024, 1027, 4100])
def test_rms_norm_batch_independence(L):
    """The same row in two launches that differ in V, in the number of rows and in the row's position: equal bytes in both results,
    and in the statistic; two runs of one launch are equal."""
    Ma, xa, gamma = R.make_rows(5 * L, 1, 2, L)
    Mb, xb, _ = R.make_rows(5 * L + 1, 3, 5, L)
    ra, (vb, rb) = 1, (2, 3)
    Mb[vb, rb], xb[rb] = Ma[0, ra], xa[ra]
    sa, sb = R.fp32_stats(xa), R.fp32_stats(xb)
    sb[rb] = sa[ra]
    A, B, B2 = run_rules(Ma, xa, gamma, sa), run_rules(Mb, xb, gamma, sb), run_rules(Mb, xb, gamma, sb)
    for a, b, b2 in zip(A, B, B2):
        assert torch.equal(a[0, ra], b[vb, rb]) and torch.equal(b, b2)
    assert kernels.rms_norm_stats(xa.to(DEV), 2, R.RMS_EPS)[ra] == kernels.rms_norm_stats(xb.to(DEV), 5, R.RMS_EPS)[rb]


def test_rms_norm_rules_with_statistics_of_the_kernel():
    """Both launches in a row, as the extension calls them, against torch's own RMSNorm backward in fp64."""
    L, rows, V = 1027, 3, 2
    M, x, gamma = R.make_rows(3, V, rows, L)
    rstd = kernels.rms_norm_stats(x.to(DEV), rows, R.RMS_EPS)
    refs, mags = R.rules(M, x, gamma, rstd.cpu())
    out, w = kernels.rms_norm_rules(M.to(DEV), x.to(DEV), gamma.to(DEV), rstd)
    check(out, refs[0], R.rules_bounds(mags, L, vec=False)[0], "out")
    xr = x.double().requires_grad_(True)
    y = torch.nn.functional.rms_norm(xr, (L,), gamma.double(), R.RMS_EPS)
    auto = torch.stack([torch.autograd.grad(y, xr, M[v].double(), retain_graph=True)[0] for v in range(V)])
    assert torch.allclose(out.cpu().double(), auto, rtol=1e-4, atol=1e-5 * auto.abs().max().item())


@pytest.mark.parametrize("D,A,V", R.POSITION_CASES)
def test_rms_norm_position_sums(D, A, V):
    N = 3
    g = R.gen(D + 10 * A + V)
    M, x = R.generic(g, V, N, A, D), R.generic(g, N, A, D)
    rstd = R.fp32_stats(x.view(N * A, D))
    ref, bound = R.position_sums(M, x, rstd)
    buf, view = R.guarded((V, N, D), DEV)
    pw = kernels.rms_norm_position_sums(M.to(DEV), x.to(DEV), rstd.to(DEV), out=view)
    assert R.guards_intact(buf, view)
    check(pw, ref, bound, "pw")
    # sample 1 alone (V = 1, N = 1): the same bytes
    pw1 = kernels.rms_norm_position_sums(M[V - 1:, 1:2].to(DEV), x[1:2].to(DEV), rstd[A:2 * A].to(DEV))
    assert torch.equal(pw1[0, 0], pw[V - 1, 1])


# ---- gate -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [False, True], ids=["aligned", "offset4"])
@pytest.mark.parametrize("V", R.VS)
@pytest.mark.parametrize("n", R.GATE_N)
def test_gate(n, V, shift):
    g = R.gen(n + V)
    M, a, b = R.generic(g, V, n), R.generic(g, n), R.generic(g, n)
    Md, ad, bd = dev(M, shift), a.to(DEV), b.to(DEV)
    for want in ((True, True), (True, False), (False, True)):
        bufs = [R.guarded((V, n), DEV) if w else (None, None) for w in want]
        Ga, Gb = kernels.gate_jac_t(Md, ad if want[1] else None, bd if want[0] else None, want, out_a=bufs[0][1], out_b=bufs[1][1])
        for (buf, view), got, other in zip(bufs, (Ga, Gb), (b, a)):
            if view is None:
                assert got is None
            else:
                assert R.guards_intact(buf, view) and torch.equal(got.cpu(), M * other)      # torch's fp32 product, bit for bit
    # every operand offset in turn (the scalar body), and a [V, N, F] factor
    for which in range(2):
        Ga, Gb = kernels.gate_jac_t(M.to(DEV), dev(a, which == 0), dev(b, which == 1))
        assert torch.equal(Ga.cpu(), M * b) and torch.equal(Gb.cpu(), M * a)


def test_gate_many_elements_and_slices():
    """More slices than the rows of workgroups one launch spreads them over (V = 5000 of 8 elements), a [V, N, F] factor, and a
    slice of more positions than one trip of the launch takes (32 768 workgroups of 256)."""
    for V, shape in ((5000, (8,)), (2, (3, 70001)), (1, (32768 * 256 + 5,))):
        g = R.gen(V)
        M, a, b = (torch.randn(*s_, generator=g) for s_ in ((V, *shape), shape, shape))
        Ga, Gb = kernels.gate_jac_t(M.to(DEV), a.to(DEV), b.to(DEV))
        assert torch.equal(Ga.cpu(), M * b) and torch.equal(Gb.cpu(), M * a)


# ---- rotary ---------------------------------------------------------------------------------------------------------------------------
def rope_case(d, T, H, Rr):
    g = R.gen(d + 10 * T + H + Rr)
    return R.generic(g, Rr, T, 3 * H * d), R.rope_tables(T, d)


@pytest.mark.parametrize("mode", ["out_of_place", "in_place", "offset4"])
@pytest.mark.parametrize("d,T,H,Rr", R.ROPE_CASES)
def test_rope(d, T, H, Rr, mode):
    M, (cos, sin) = rope_case(d, T, H, Rr)
    ref, bound = R.rope(M, cos, sin, H)
    shift = mode == "offset4"
    Md = dev(M, shift)
    if mode == "in_place":
        buf, view = R.guarded(M.shape, DEV)
        view.copy_(Md)
        G = kernels.rope_jac_t(view, cos.to(DEV), sin.to(DEV), H, out=view)
    else:
        buf, view = R.guarded(M.shape, DEV, shift)
        G = kernels.rope_jac_t(Md, cos.to(DEV), sin.to(DEV), H, out=view)
        assert torch.equal(Md.cpu(), M)                                        # the input is left alone
    assert G is view and R.guards_intact(buf, view, shift)
    check(G, ref, bound, f"d={d} T={T} H={H} R={Rr} {mode}")
    assert torch.equal(G.cpu()[..., 2 * H * d:], M[..., 2 * H * d:])               # the v third: bit for bit
    if T > 1:
        assert not torch.equal(G.cpu()[:, 1:, :2 * H * d], M[:, 1:, :2 * H * d])
    # a factor with leading dimensions [V, N, T, 3 E] is R = V N rows
    if Rr == 6:
        assert torch.equal(kernels.rope_jac_t(M.view(2, 3, T, -1).to(DEV), cos.to(DEV), sin.to(DEV), H).view(Rr, T, -1), G)


@pytest.mark.parametrize("d,T,H", [(2, 5, 1), (6, 33, 3), (64, 33, 3), (130, 5, 1)])
def test_rope_rule_inverts_the_forward_pass(d, T, H):
    """A rotation's transpose is its inverse: the rule applied to the module's forward output returns the input, with the module's
    own tables (computed on the device)."""
    x = R.generic(R.gen(d + T), 4, T, 3 * H * d)
    mod = RotaryEmbedding(H)
    y = mod(x.to(DEV))
    back = kernels.rope_jac_t(y, *mod.tables(T, d, DEV, torch.float32), H)
    check(back, x.double(), R.rope_roundtrip_bound(x, H), "round trip")
    assert torch.equal(back.cpu()[..., 2 * H * d:], x[..., 2 * H * d:])
    # and the rule itself with those tables against fp64
    cos, sin = (t.cpu() for t in mod.tables(T, d, DEV, torch.float32))
    ref, bound = R.rope(x, cos, sin, H)
    check(kernels.rope_jac_t(x.to(DEV), *mod.tables(T, d, DEV, torch.float32), H), ref, bound, "rule")


def test_rope_many_rows():
    """70 000 (r, t) rows of one pair and one copied pair (64 rows per workgroup), and 33 000 rows of 260 work items each: more than
    one trip of the launch's 32 768 workgroups at one row each."""
    for d, T, Rr in ((2, 7, 10000), (130, 33, 1000)):
        M, (cos, sin) = torch.randn(Rr, T, 3 * d, generator=R.gen(d)), R.rope_tables(T, d)
        ref, bound = R.rope(M, cos, sin, 1)
        check(kernels.rope_jac_t(M.to(DEV), cos.to(DEV), sin.to(DEV), 1), ref, bound, f"many rows d={d}")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_launchers_refuse_bad_arguments():
    M, x = torch.zeros(2, 4, 6, device=DEV), torch.zeros(4, 6, device=DEV)
    rstd = torch.zeros(4, device=DEV)
    canary = torch.full((64,), 7.0, device=DEV)
    with pytest.raises(ValueError):
        kernels.rms_norm_rules(M, x[:3], None, rstd)
    with pytest.raises(ValueError):
        kernels.rms_norm_rules(M, x, torch.zeros(5, device=DEV), rstd)
    with pytest.raises(ValueError):
        kernels.rms_norm_rules(M, x, None, rstd, want=(False, False))
    with pytest.raises(ValueError):
        kernels.rms_norm_rules(M, x, None, rstd, out=torch.zeros(2, 4, 5, device=DEV))
    with pytest.raises(ValueError):
        kernels.rms_norm_position_sums(M, x, rstd)
    with pytest.raises(RuntimeError):
        kernels.rms_norm_stats(x.cpu(), 4, 1e-5)
    with pytest.raises(ValueError):
        kernels.gate_jac_t(M, x, x[:3])
    with pytest.raises(ValueError):
        kernels.gate_jac_t(M, x, None)
    with pytest.raises(ValueError):
        kernels.rope_jac_t(torch.zeros(2, 4, 18, device=DEV), torch.zeros(4, 1, device=DEV), torch.zeros(4, 1, device=DEV), 2)   # d = 3
    with pytest.raises(ValueError):
        kernels.rope_jac_t(torch.zeros(2, 4, 24, device=DEV), torch.zeros(3, 2, device=DEV), torch.zeros(3, 2, device=DEV), 2)   # tables of T = 3
    big = torch.zeros(2, 4, 24, device=DEV)
    with pytest.raises(ValueError):
        kernels.rope_jac_t(big[:1], torch.zeros(4, 2, device=DEV), torch.zeros(4, 2, device=DEV), 2, out=big.view(-1)[4:100].view(1, 4, 24))
    lib = _lib.load()
    p = canary.data_ptr()
    assert lib.vivit_rms_norm_rules_f32(M.data_ptr(), x.data_ptr(), None, rstd.data_ptr(), None, None, 2, 4, 6, None) == _lib.VIVIT_E_BADARG
    assert lib.vivit_rms_norm_rules_f32(M.data_ptr(), x.data_ptr(), None, rstd.data_ptr(), p, None, -1, 4, 6, None) == _lib.VIVIT_E_BADARG
    assert lib.vivit_rms_norm_rules_f32(M.data_ptr(), x.data_ptr(), None, rstd.data_ptr(), p, None, 0, 4, 6, None) == _lib.VIVIT_OK
    assert lib.vivit_gate_jac_t_f32(M.data_ptr(), None, None, None, None, 2, 24, None) == _lib.VIVIT_E_BADARG
    assert lib.vivit_gate_jac_t_f32(M.data_ptr(), None, None, p, None, 2, 24, None) == _lib.VIVIT_E_BADARG
    assert lib.vivit_gate_jac_t_f32(M.data_ptr(), x.data_ptr(), x.data_ptr(), p, None, 0, 24, None) == _lib.VIVIT_OK
    assert lib.vivit_rope_jac_t_f32(M.data_ptr(), x.data_ptr(), x.data_ptr(), p, 1, 1, 1, 3, None) == _lib.VIVIT_E_BADARG
    assert lib.vivit_rope_jac_t_f32(M.data_ptr(), x.data_ptr(), x.data_ptr(), p, 1, 0, 1, 2, None) == _lib.VIVIT_OK
    assert lib.vivit_rms_norm_stats_f32(x.data_ptr(), p, 4, 6, -1.0, None) == _lib.VIVIT_E_BADARG
    torch.cuda.synchronize()
    assert bool((canary == 7.0).all())    # no launch wrote anything
