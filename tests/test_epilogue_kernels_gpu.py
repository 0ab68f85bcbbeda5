"""The small kernels around the GEMMs and the eigensolver, one by one against the fp64 references of
tests/epilogue_refs.py at the shapes where their code paths change: vector / scalar bodies (sizes % 4, pointers that are
only 4-byte aligned), the unrolled main loop and ragged tail of the row reductions, the second trip of every grid-stride
loop, the 65 535-row launch split and several chunks per row of the row norms, padded leading dimensions, alpha / beta.

Each case runs the exact family (small integers: the fp32 result must equal the fp64 reference bit for bit, whatever the
summation order -- a dropped, duplicated or misindexed element shows) and the generic family under the derived error
bounds stated in tests/epilogue_refs.py.  The test id names the kernel body a shape takes."""
import math

import pytest
import torch

import epilogue_refs as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FAMILIES = ["exact", "generic"]
F64 = torch.float64


def dev(*ts):
    return [t.to(DEV) for t in ts]


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def check(family, got, ref, bound):
    """exact family: equality with the fp64 reference; generic family: ``|got - ref| <= bound`` elementwise."""
    if family == "exact":
        assert torch.equal(got.to(F64), ref.to(got.device))
    else:
        ok, msg = R.within(got, ref.to(got.device), bound.to(got.device))
        assert ok, msg


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


# ---- gram_hadamard ---------------------------------------------------------------------------------------------------------
def _had_id(C, N):
    return f"{'vec' if N % 4 == 0 else 'scalar'}{'-stride' if (C * N) ** 2 // (4 if N % 4 == 0 else 1) > 524288 else ''}-C{C}-N{N}"


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("alpha,beta", R.HADAMARD_AB, ids=lambda v: f"{v:g}")
@pytest.mark.parametrize("C,N", R.HADAMARD_SHAPES, ids=[_had_id(*s) for s in R.HADAMARD_SHAPES])
def test_gram_hadamard(C, N, alpha, beta, family):
    from vivit_amd import kernels

    Gz, Gs, G0 = dev(*R.make_hadamard(family, C, N))
    ref = R.hadamard(Gz, Gs, C, N, alpha, beta, G0)
    bound = R.hadamard_bound(R.hadamard(Gz.abs(), Gs.abs(), C, N, abs(alpha), abs(beta), G0.abs()))
    if beta == 0.0:
        check(family, kernels.gram_hadamard(Gz, Gs, C, N, alpha=alpha), ref, bound)
        out = torch.full_like(G0, float("nan"))   # beta = 0 must not read the old contents
    else:
        out = G0.clone()
    res = kernels.gram_hadamard(Gz, Gs, C, N, out=out, alpha=alpha, beta=beta)
    assert res is out
    check(family, out, ref, bound)


@pytest.mark.parametrize("which", ["Gz", "Gs", "out"])
@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("C,N", [(2, 8), (5, 64)])
def test_gram_hadamard_misaligned(C, N, beta, which):
    """A pointer that is only 4-byte aligned sends a shape with N % 4 == 0 to the scalar body: same bits as the aligned call."""
    from vivit_amd import kernels

    for family in FAMILIES:
        Gz, Gs, G0 = dev(*R.make_hadamard(family, C, N))
        want = kernels.gram_hadamard(Gz, Gs, C, N, out=G0.clone(), alpha=0.5, beta=beta)
        ops = {"Gz": Gz, "Gs": Gs, "out": G0.clone()}
        ops[which] = R.misaligned(ops[which])
        got = kernels.gram_hadamard(ops["Gz"], ops["Gs"], C, N, out=ops["out"], alpha=0.5, beta=beta)
        assert got.data_ptr() == ops["out"].data_ptr()
        assert same_bits(got, want), f"scalar-misaligned-{which} differs from the aligned call ({family})"
        check(family, got, R.hadamard(Gz, Gs, C, N, 0.5, beta, G0),
              R.hadamard_bound(R.hadamard(Gz.abs(), Gs.abs(), C, N, 0.5, beta, G0.abs())))


# ---- gram_hadamard_block -----------------------------------------------------------------------------------------------------
def _block_cases():
    for name, Cr, Nr, Cc, Nc in R.HADAMARD_BLOCK_SHAPES:
        for pad in (0, 4, 3):
            ldg = Cc * Nc + pad
            body = "vec" if Nc % 4 == 0 and ldg % 4 == 0 else "scalar"
            yield pytest.param(Cr, Nr, Cc, Nc, ldg, id=f"{name}-ldg+{pad}-{body}")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("Cr,Nr,Cc,Nc,ldg", list(_block_cases()))
def test_gram_hadamard_block(Cr, Nr, Cc, Nc, ldg, beta, family):
    from vivit_amd import kernels

    rows, cols = Cr * Nr, Cc * Nc
    Gz, Gs, G0 = dev(*R.make_hadamard_block(family, Cr, Nr, Cc, Nc))
    alpha = 0.5
    buf, view = R.with_sentinel_padding(rows, cols, ldg, DEV)
    view.copy_(G0 if beta != 0.0 else torch.full_like(G0, float("nan")))
    before = buf.clone()
    res = kernels.gram_hadamard_block(Gz, Gs, Cr, Nr, Cc, Nc, out=view, alpha=alpha, beta=beta)
    assert res is view
    assert R.padding_untouched(buf, cols) and same_bits(buf[:, cols:], before[:, cols:])
    ref = R.hadamard_block(Gz, Gs, Cr, Nr, Cc, Nc, alpha, beta, G0)
    bound = R.hadamard_bound(R.hadamard_block(Gz.abs(), Gs.abs(), Cr, Nr, Cc, Nc, alpha, beta, G0.abs()))
    check(family, view, ref, bound)
    if beta == 0.0 and ldg == cols:
        check(family, kernels.gram_hadamard_block(Gz, Gs, Cr, Nr, Cc, Nc, alpha=alpha), ref, bound)


@pytest.mark.parametrize("which", ["Gz", "Gs", "out"])
@pytest.mark.parametrize("name,Cr,Nr,Cc,Nc", [s for s in R.HADAMARD_BLOCK_SHAPES if s[0] in ("vtg-vec", "blockrow-vec")])
def test_gram_hadamard_block_misaligned(name, Cr, Nr, Cc, Nc, which):
    from vivit_amd import kernels

    for family in FAMILIES:
        Gz, Gs, G0 = dev(*R.make_hadamard_block(family, Cr, Nr, Cc, Nc))
        want = kernels.gram_hadamard_block(Gz, Gs, Cr, Nr, Cc, Nc, out=G0.clone(), alpha=2.0, beta=1.0)
        ops = {"Gz": Gz, "Gs": Gs, "out": G0.clone()}
        ops[which] = R.misaligned(ops[which])
        got = kernels.gram_hadamard_block(ops["Gz"], ops["Gs"], Cr, Nr, Cc, Nc, out=ops["out"], alpha=2.0, beta=1.0)
        assert same_bits(got, want), f"scalar-misaligned-{which} differs from the aligned call ({family})"
        check(family, got, R.hadamard_block(Gz, Gs, Cr, Nr, Cc, Nc, 2.0, 1.0, G0),
              R.hadamard_bound(R.hadamard_block(Gz.abs(), Gs.abs(), Cr, Nr, Cc, Nc, 2.0, 1.0, G0.abs())))


# ---- class_contract / class_expand -------------------------------------------------------------------------------------------
def _class_id(s):
    F, C, N, O = s
    return f"F{F}-C{C}-N{N}-O{O}{'-stride' if max(F * O * N, F * C * N) > 524288 else ''}"


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("F,C,N,O", R.CLASS_SHAPES, ids=[_class_id(s) for s in R.CLASS_SHAPES])
def test_class_contract_expand(F, C, N, O, family):
    from vivit_amd import kernels

    mat, s, U = dev(*R.make_class(family, F, C, N, O))
    T = kernels.class_contract(mat, s)
    assert T.shape == (F, O, N)
    check(family, T, R.class_contract(mat, s), R.sum_bound(C, R.class_contract(mat.abs(), s.abs())))
    Rr = kernels.class_expand(s, U)
    assert Rr.shape == (F, C, N)
    check(family, Rr, R.class_expand(s, U), R.sum_bound(O, R.class_expand(s.abs(), U.abs())))


def test_class_contract_expand_non_contiguous():
    """The wrappers copy non-contiguous operands: same bits as with contiguous ones."""
    from vivit_amd import kernels

    F, C, N, O = 3, 5, 13, 7
    mat, s, U = dev(*R.make_class("generic", F, C, N, O))
    mat_nc = mat.transpose(1, 2).contiguous().transpose(1, 2)
    s_nc = torch.stack([s, s], 3)[..., 0]
    U_nc = U.transpose(0, 2).contiguous().transpose(0, 2)
    assert not (mat_nc.is_contiguous() or s_nc.is_contiguous() or U_nc.is_contiguous())
    assert same_bits(kernels.class_contract(mat_nc, s_nc), kernels.class_contract(mat, s))
    assert same_bits(kernels.class_expand(s_nc, U_nc), kernels.class_expand(s, U))


# ---- dir_curvature -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("C,N,K", R.DIR_CURV_SHAPES, ids=[f"C{c}-N{n}-K{k}{'-stride' if n * k > 524288 else ''}" for c, n, k in R.DIR_CURV_SHAPES])
def test_dir_curvature(C, N, K, family):
    from vivit_amd import kernels

    GE, ev = dev(*R.make_dir_curvature(family, C, N, K))
    scale = 0.25
    got = kernels.dir_curvature(GE, ev, C, N, scale)
    assert got.shape == (N, K)
    ref = R.dir_curvature(GE, ev, C, N, scale)
    check(family, got, ref, (C + 2) * R.EPS * ref + 4 * R.EPS * ref)   # (all terms non-negative: sum|terms| = ref)
    # GE as a non-contiguous slice: the wrapper copies it
    wide = torch.cat([GE, GE + 1.0], 1)
    assert not wide[:, :K].is_contiguous() or K == wide.shape[1] or C * N == 1
    assert same_bits(kernels.dir_curvature(wide[:, :K], ev, C, N, scale), got)


def test_dir_curvature_zero_eigenvalue():
    """IEEE fp32 division, as the reference's: x / 0 = inf, 0 / 0 = NaN."""
    from vivit_amd import kernels

    C, N, K = 2, 6, 7
    GE, ev = dev(*R.make_dir_curvature("exact", C, N, K))
    ev[3] = 0.0
    GE.view(C, N, K)[:, 2, 3] = 0.0     # sample 2: 0 / 0
    GE.view(C, N, K)[0, 4, 3] = 3.0     # sample 4: 9 or more / 0
    got = kernels.dir_curvature(GE, ev, C, N, 0.5)
    ref = R.dir_curvature(GE, ev, C, N, 0.5)
    assert math.isnan(float(got[2, 3])) and math.isnan(float(ref[2, 3]))
    assert float(got[4, 3]) == float("inf") == float(ref[4, 3])
    assert torch.equal(got.to(F64).nan_to_num(nan=-1.0), ref.nan_to_num(nan=-1.0))


# ---- scale_cols_rsqrt_ ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("pre", [1.0, 0.5])
@pytest.mark.parametrize("rows,K,ldx", R.SCALE_COLS_SHAPES,
                         ids=[f"rows{r}-K{k}-ldx{l}{'-stride' if r * k > 524288 else ''}" for r, k, l in R.SCALE_COLS_SHAPES])
def test_scale_cols_rsqrt(rows, K, ldx, pre, family):
    from vivit_amd import kernels

    X, ev = dev(*R.make_scale_cols(family, rows, K))
    buf, view = R.with_sentinel_padding(rows, K, ldx, DEV)
    view.copy_(X)
    res = kernels.scale_cols_rsqrt_(view, ev, pre)
    assert res is view
    assert R.padding_untouched(buf, K)
    ref = R.scale_cols_rsqrt(X, ev, pre)
    check(family, view, ref, 4 * R.EPS * ref.abs())


# ---- normalize_rows_ (vivit_row_sqnorm_acc_f32 + vivit_scale_rows_rsqrt_f32) -----------------------------------------------------
def _norm_id(s):
    K, lens = s
    nch = max(-(-ln // 8192) for ln in lens)
    return f"K{K}{'-split' if K > 65535 else ''}-len{'+'.join(map(str, lens))}-chunks{nch}"


@pytest.mark.parametrize("K,lens", R.NORMALIZE_SHAPES, ids=[_norm_id(s) for s in R.NORMALIZE_SHAPES])
def test_row_sqnorm_acc_exact(K, lens):
    """``acc[k] += ||X[k]||^2`` through the C entry point with a caller-supplied, pre-filled ``acc``, tensor after tensor:
    the accumulated squares bit for bit; the workspace query is ``K ceil(len / 8192) 4`` bytes."""
    from vivit_amd import _lib

    lib = _lib.load()
    ts = dev(*R.make_normalize("exact", K, lens))
    acc0 = (torch.arange(K, device=DEV) % 1000).float()
    acc = acc0.clone()
    for t, ln in zip(ts, lens):
        need = lib.vivit_row_sqnorm_workspace_bytes(K, ln)
        assert need == K * (-(-ln // 8192)) * 4
        ws = torch.full((need // 4,), float("nan"), device=DEV)
        _lib.check(lib.vivit_row_sqnorm_acc_f32(t.data_ptr(), acc.data_ptr(), K, ln, ws.data_ptr(), need, stream()), "row_sqnorm")
        assert lib.vivit_row_sqnorm_acc_f32(t.data_ptr(), acc.data_ptr(), K, ln, ws.data_ptr(), need - 1, stream()) == _lib.VIVIT_E_WORKSPACE
    torch.cuda.synchronize()
    assert torch.equal(acc.to(F64), R.row_sqnorm(ts, acc0))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("K,lens", R.NORMALIZE_SHAPES, ids=[_norm_id(s) for s in R.NORMALIZE_SHAPES])
def test_normalize_rows(K, lens, family):
    from vivit_amd import kernels

    ts = dev(*R.make_normalize(family, K, lens))
    if len(lens) > 1:
        ts[1] = ts[1].reshape(K, -1, 2 if lens[1] % 2 == 0 else 1)   # parameter-list format: [K, *param.shape]
    refs = R.normalize_rows(ts)
    got = kernels.normalize_rows_([t.clone() for t in ts])
    total = sum(lens)
    # the squared norm is a sum of `total` non-negative terms plus one add per tensor: relative error (total + T + 2) eps;
    # rsqrt and the scaling: 4 eps relative on top
    rel = (total + len(lens) + 2) * R.EPS + 4 * R.EPS
    for g, r in zip(got, refs):
        ok, msg = R.within(g, r, rel * r.abs())
        assert ok, msg
    unit = sum((g.to(F64).reshape(K, -1) ** 2).sum(1) for g in got)
    worst = float((unit - 1.0).abs().max())
    limit = 4 * R.EPS * (1 + math.log2(total))
    print(f"max |sum_t ||t[k]||^2 - 1| = {worst:.3e} (limit {limit:.3e})")
    assert worst <= limit


# ---- vivit_symmetrize_lower_f32 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("n", R.SYMM_N)
def test_symmetrize_lower(n, pad):
    from vivit_amd import _lib

    buf, view = R.make_symm(n, n + pad)
    buf = buf.to(DEV)
    view = buf[:, :n]
    before = buf.clone()
    _lib.check(_lib.load().vivit_symmetrize_lower_f32(buf.data_ptr(), n, n + pad, stream()), "vivit_symmetrize_lower_f32")
    torch.cuda.synchronize()
    low = torch.tril(torch.ones(n, n, dtype=torch.bool, device=DEV))
    assert same_bits(view[low], before[:, :n][low]), "the lower triangle changed"
    assert torch.equal(view.to(F64), R.symmetrize_lower(before[:, :n])), "the upper triangle is not the mirror"
    assert R.padding_untouched(buf, n)


# ---- linear_weight_mjp ---------------------------------------------------------------------------------------------------------
def _fp32_outer(s, z):
    return s.unsqueeze(3) * z.view(1, z.shape[0], 1, z.shape[1])   # the same single fp32 product per element


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name,C,N,O,I", R.LINEAR_MJP_SHAPES, ids=[s[0] for s in R.LINEAR_MJP_SHAPES])
def test_linear_weight_mjp(name, C, N, O, I, family):
    from vivit_amd import kernels

    s, z = dev(*R.make_linear_mjp(family, C, N, O, I))
    got = kernels.linear_weight_mjp(s, z)
    assert got.shape == (C, N, O, I)
    assert same_bits(got, _fp32_outer(s, z))
    check(family, got, R.linear_weight_mjp(s, z), R.EPS * R.linear_weight_mjp(s, z).abs())
    # z only 4-byte aligned: the scalar body, same bits
    assert same_bits(kernels.linear_weight_mjp(s, R.misaligned(z)), got), "scalar-misaligned-z"


def test_linear_weight_mjp_grid_stride():
    """20 971 520 float4 items against a launch of 65 536 x 256 threads: the second trip of the grid-stride loop."""
    from vivit_amd import kernels

    C, N, O, I = R.LINEAR_MJP_STRIDE
    assert C * N * O * I // 4 > 65536 * 256
    s, z = dev(*R.make_linear_mjp("exact", C, N, O, I))
    got = kernels.linear_weight_mjp(s, z)
    want = _fp32_outer(s, z)
    ok = torch.equal(got, want)
    del got, want
    torch.cuda.empty_cache()
    assert ok


# ---- row_dot -------------------------------------------------------------------------------------------------------------------
def _row_dot_checks(family, M, X, rows_x, L):
    from vivit_amd import kernels

    rows = M.shape[0]
    got = kernels.row_dot(M, X, rows_x)
    assert got.shape == (rows,)
    check(family, got, R.row_dot(M, X, rows_x), R.sum_bound(L, R.row_dot(M.abs(), X.abs(), rows_x)))
    got1 = kernels.row_dot(M)
    check(family, got1, R.row_dot(M), R.sum_bound(L, R.row_dot(M.abs())))
    return got, got1


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("rows", R.ROW_ROWS)
@pytest.mark.parametrize("L", list(R.ROW_L), ids=[f"{b}-L{l}" for l, b in R.ROW_L.items()])
def test_row_dot(L, rows, family):
    M, X = dev(*R.make_rows(family, rows, rows, L))
    _row_dot_checks(family, M, X, rows, L)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("L", list(R.ROW_L), ids=[f"{b}-L{l}" for l, b in R.ROW_L.items()])
def test_row_dot_shared_x_and_misaligned(L, family):
    """``rows_x < rows`` (X shared by the slices) and operands that are only 4-byte aligned (scalar body for every L)."""
    from vivit_amd import kernels

    M, X = dev(*R.make_rows(family, 12, 4, L))
    _row_dot_checks(family, M, X, 4, L)
    for Mm, Xm, what in ((R.misaligned(M), X, "M"), (M, R.misaligned(X), "X")):
        got = kernels.row_dot(Mm, Xm, 4)
        check(family, got, R.row_dot(M, X, 4), R.sum_bound(L, R.row_dot(M.abs(), X.abs(), 4)))
    got = kernels.row_dot(R.misaligned(M))
    check(family, got, R.row_dot(M), R.sum_bound(L, R.row_dot(M.abs())))


# ---- bn_eval_rules -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("C", [1, 7])
@pytest.mark.parametrize("L", list(R.ROW_L), ids=[f"{b}-L{l}" for l, b in R.ROW_L.items()])
def test_bn_eval_rules(L, C, V, family):
    from vivit_amd import kernels

    N = 2
    M, x, scale, mean, rstd = dev(*R.make_bn(family, V, N, C, L))
    rout, rmx, rms = R.bn_eval_rules(M, x, scale)
    _, amx, ams = R.bn_eval_rules(M.abs(), x.abs(), scale)
    out, mx, ms = kernels.bn_eval_rules(M, x, scale)
    assert out.shape == M.shape and mx.shape == ms.shape == (V, N, C)
    check(family, out, rout, R.EPS * rout.abs())
    assert same_bits(out, M * scale.view(1, 1, C, 1))   # one fp32 product per element
    check(family, mx, rmx, R.sum_bound(L, amx))
    check(family, ms, rms, R.sum_bound(L, ams))
    # the header's promise: the sums are those of vivit_row_dot_f32 on the same operands, bit for bit
    assert same_bits(mx.reshape(-1), kernels.row_dot(M.reshape(-1, L), x.reshape(-1, L), N * C))
    assert same_bits(ms.reshape(-1), kernels.row_dot(M.reshape(-1, L)))
    # with mean / rstd: the finished weight rule; the other two outputs as before
    out2, w, ms2 = kernels.bn_eval_rules(M, x, scale, mean, rstd)
    assert same_bits(out2, out) and same_bits(ms2, ms)
    rw = R.bn_eval_rules(M, x, scale, mean, rstd)[1]
    check(family, w, rw, R.bn_weight_bound(L, amx, ams, mean, rstd))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("L", list(R.ROW_L), ids=[f"{b}-L{l}" for l, b in R.ROW_L.items()])
def test_bn_eval_rules_misaligned(L, family):
    """M or x only 4-byte aligned: the scalar body for every L.  mx equals row_dot of the same (misaligned) operands bit for
    bit; msum equals row_dot of M taken through the same body (row_dot without X looks at M's alignment only, so for a
    misaligned x it is handed a misaligned copy of M)."""
    from vivit_amd import kernels

    V, N, C = 3, 2, 7
    M, x, scale, mean, rstd = dev(*R.make_bn(family, V, N, C, L))
    rout, rmx, rms = R.bn_eval_rules(M, x, scale)
    _, amx, ams = R.bn_eval_rules(M.abs(), x.abs(), scale)
    for Mm, xm, what in ((R.misaligned(M), x, "M"), (M, R.misaligned(x), "x")):
        out, mx, ms = kernels.bn_eval_rules(Mm, xm, scale)
        check(family, out, rout, R.EPS * rout.abs())
        check(family, mx, rmx, R.sum_bound(L, amx))
        check(family, ms, rms, R.sum_bound(L, ams))
        assert same_bits(mx.reshape(-1), kernels.row_dot(Mm.reshape(-1, L), xm.reshape(-1, L), N * C)), f"scalar-misaligned-{what}"
        assert same_bits(ms.reshape(-1), kernels.row_dot(R.misaligned(M).reshape(-1, L))), f"scalar-misaligned-{what}"
        w = kernels.bn_eval_rules(Mm, xm, scale, mean, rstd)[1]
        check(family, w, R.bn_eval_rules(M, x, scale, mean, rstd)[1], R.bn_weight_bound(L, amx, ams, mean, rstd))


@pytest.mark.parametrize("skip", ["out", "mx", "msum"])
@pytest.mark.parametrize("L", [20, 257, 516], ids=["vec-tail-L20", "scalar-L257", "vec-main+tail-L516"])
def test_bn_eval_rules_null_outputs(L, skip):
    """vivit_bn_eval_rules_f32 with one of out / mx / msum NULL: the remaining outputs bit for bit those of the full call."""
    from vivit_amd import _lib, kernels

    V, N, C = 3, 2, 7
    M, x, scale, _, _ = dev(*R.make_bn("generic", V, N, C, L))
    full = dict(zip(("out", "mx", "msum"), kernels.bn_eval_rules(M, x, scale)))
    got = {"out": torch.full_like(M, float("nan")), "mx": torch.full((V, N, C), float("nan"), device=DEV),
           "msum": torch.full((V, N, C), float("nan"), device=DEV)}
    ptr = {k: (None if k == skip else t.data_ptr()) for k, t in got.items()}
    st = _lib.load().vivit_bn_eval_rules_f32(M.data_ptr(), x.data_ptr(), scale.data_ptr(), ptr["out"], ptr["mx"], ptr["msum"],
                                             V * N * C, N * C, C, L, None, None, stream())
    _lib.check(st, "vivit_bn_eval_rules_f32")
    torch.cuda.synchronize()
    for k in got:
        if k == skip:
            assert bool(got[k].isnan().all())
        else:
            assert same_bits(got[k], full[k]), k
