"""The lowerings of the convolution family (vivit_amd/backend/extensions.py) on the CPU, with the four 2-D entry points
replaced by the fp64 stand-ins of tests/conv_family_refs.py: the index arithmetic above the kernels against fp64 autograd,
BIT FOR BIT on integer data.  No GPU.

* every case of the exact family equals its reference; ``served`` is what the lowering returns; the 2-D geometry the lowering
  hands to the kernels has the planner route the case is labelled with (mirrors of tests/conv_refs.py) -- a planner or lowering
  change that moves a case off its branch fails here until the case follows; sum|terms| stays below 2^24;
* a seeded sweep of 300 random geometries per lowering (kernels 1-3, strides 1-4, paddings 0-3, dilations 1-3, groups 1-3,
  every admissible output padding, sizes down to 1, taps wholly in the padding), nothing skipped but what torch rejects;
* the try / except of ``_jac_t_mat_prod``: VIVIT_E_UNSUPPORTED falls through to the generic rule, any other status propagates.
"""
import pytest
import torch

import conv_family_refs as CF
import conv_refs as R
from vivit_amd import _lib
from vivit_amd.backend import extensions as ext

F64 = torch.float64
EXACT_RUNS = [(n, r) for n, r, f in CF.RUNS if f == "exact"]


@pytest.fixture
def standins(monkeypatch):
    return CF.StandIns().install(monkeypatch)


def assert_equal(got, ref, what):
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} for {tuple(ref.shape)}"
    bad = got.double() != ref
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} entries differ, first at {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("name,rule", EXACT_RUNS)
def test_lowering_equals_fp64_autograd(name, rule, standins):
    case = CF.ALL[name]
    module, x, M = CF.on_device(case, "exact", "cpu", F64)
    got = CF.lower(case, rule, module, M, x)
    if rule == "input" and case.expects["served"] is None:
        assert got is None, f"{case.expects['lowering']} serves a case labelled as declined ({case.expects['reason']})"
        return
    assert got is not None, f"{case.expects['lowering']} declined a case labelled as served"
    ref, mag = CF.reference(name, rule, "exact")
    assert_equal(got, ref, f"{name}/{rule}")
    assert got.dtype == F64
    for d in case.expects["zero_depth"] if rule == "input" else ():
        assert torch.count_nonzero(got[:, :, :, d]) == 0


@pytest.mark.parametrize("name", [c.name for c in CF.CASES if CF.is_conv(c.kind)])
def test_case_takes_the_route_it_is_labelled_with(name, standins):
    """The 2-D geometry of every launch (e.g. Geom(Ci, Cc, QD Hp + tail, W, (KH, KW), (sh, sw), (0, pw), (dh, dw)) with OH = QD
    QHp for the 3-D weight rule) through the planner mirrors."""
    case = CF.ALL[name]
    module, x, M = CF.on_device(case, "exact", "cpu", F64)
    for rule in ("input", "weight"):
        standins.calls.clear()
        CF.lower(case, rule, module, M, x)
        want = case.expects[rule + "_route"]
        got = CF.routes(standins.calls)
        assert got == ({(rule, want)} if want else set()), f"{name}/{rule}: labelled {want}, the launches take {sorted(got)}"
        if want == "mfma" and rule == "input":   # with the matrix pipe off the scalar kernel must refuse the slice: the route is observable
            off = {R.input_plan(c.geom, mfma=False, rows=c.rows, out=c.out)["route"] for c in standins.calls}
            assert off == {"unsupported"}


@pytest.mark.parametrize("name,rule,fam", CF.RUNS)
def test_partial_sums_stay_exact_and_operands_match(name, rule, fam):
    """Precondition of the bit-for-bit comparison, and the shapes of every family's operands."""
    case = CF.ALL[name]
    ref, mag = CF.reference(name, rule, fam)
    assert bool(torch.isfinite(ref).all()) and bool((mag >= ref.abs() * (1 - 1e-12)).all())
    if fam == "exact":
        assert mag.max().item() < 2 ** 24, f"sum|terms| reaches {mag.max().item():.0f}"
        assert bool((ref == ref.round()).all()) or not CF.is_conv(case.kind)   # (averages are dyadic, not integer)
    assert CF.n_terms(case, rule) >= 1 and CF.n_terms(case, rule, True) >= 1


def test_labelled_zero_slices_are_structural():
    """``zero_depth``: with all-ones operands the reference of those depth slices is zero (and of no other slice)."""
    for case in CF.CASES:
        if not case.expects["zero_depth"]:
            continue
        W, x, M = CF.operands(case, "exact")
        ones = CF.input_rule(case, None if W is None else torch.ones_like(W), x, torch.ones_like(M))
        dead = [d for d in range(ones.shape[3]) if torch.count_nonzero(ones[:, :, :, d]) == 0]
        assert tuple(dead) == case.expects["zero_depth"], case.name


def test_case_list_covers_what_it_claims(standins):
    e = {c.name: c for c in CF.CASES}
    module, x, M = CF.on_device(e["c3-w-lds"], "exact", "cpu", F64)   # scalar because the stack is refused LDS, nothing else
    CF.lower(e["c3-w-lds"], "weight", module, M, x)
    assert {R.weight_plan(c.geom, out=c.out)["reason"] for c in standins.calls} == {"LDS"}
    from vivit_amd.backend.extensions import _depth_range

    s = e["c3-empty-tap"].spec   # tap 1 empty, taps 0 and 2 a single slice
    ranges = [_depth_range(2, 2, 3, 2, kd) for kd in range(3)]
    assert [hi - lo + 1 for lo, hi, _ in ranges] == [1, 0, 1] and s["size"][0] == 2
    assert CF.out_shape(e["c3-od1"])[2] == 1
    assert {c.expects["reason"] for c in CF.CASES if c.expects["served"] is None} == {
        "p > (K - 1) d", "Cout/G kh kw > 1024", "ceil_mode", "dilation", "count_include_pad=False", "divisor_override"}
    for rule in ("input", "weight"):
        assert any(c.expects.get(rule + "_route") == "mfma" for c in CF.CASES)
    assert len(CF.MFMA_RUNS) >= 8
    for c in CF.CASES:
        if CF.is_transposed(c.kind):
            assert CF.declines(c) == (c.expects["served"] is None), c.name


# ---- the sweep -------------------------------------------------------------------------------------------------------------
SWEEP = 300


def _draw(gen, lo, hi, n=None):
    v = torch.randint(lo, hi + 1, (n or 1,), generator=gen).tolist()
    return v[0] if n is None else tuple(v)


def _sweep_case(kind, gen, i):
    """One random geometry: kernels 1-3, strides 1-4, paddings 0-3, dilations 1-3, groups 1-3, every admissible output padding;
    the size is drawn from the smallest that gives one output position (so: sizes down to 1, taps wholly in the padding) up to
    four more.  Only what torch rejects is left to be skipped."""
    nd = CF.NDIM[kind]
    k, s, p, d = _draw(gen, 1, 3, nd), _draw(gen, 1, 4, nd), _draw(gen, 0, 3, nd), _draw(gen, 1, 3, nd)
    g = _draw(gen, 1, 3)
    cin, cout = g * _draw(gen, 1, 2), g * _draw(gen, 1, 3)
    if CF.is_transposed(kind):
        op = tuple(_draw(gen, 0, max(s_, d_) - 1) for s_, d_ in zip(s, d))
        # the smallest input whose output has one position: (q - 1) s - 2 p + d (k - 1) + op + 1 >= 1
        least = [max(1, 1 + R.cdiv(2 * p_ - d_ * (k_ - 1) - o_, s_)) for k_, s_, p_, d_, o_ in zip(k, s, p, d, op)]
        size = tuple(m + _draw(gen, 0, 3) for m in least)
        return CF.conv(f"sweep-{kind}-{i}", kind, cin, cout, k, size, s=s, p=p, d=d, g=g, op=op, N=2, V=1, lowering="sweep", edge="sweep")
    least = [max(1, d_ * (k_ - 1) + 1 - 2 * p_) for k_, p_, d_ in zip(k, p, d)]
    size = tuple(m + _draw(gen, 0, 4) for m in least)
    return CF.conv(f"sweep-{kind}-{i}", kind, cin, cout, k, size, s=s, p=p, d=d, g=g, N=2, V=1, lowering="sweep", edge="sweep")


def _sweep_pool(kind, gen, i):
    nd = CF.NDIM[kind]
    k = _draw(gen, 1, 3, nd) if kind.startswith("max") else tuple(2 ** e for e in _draw(gen, 0, 2, nd))   # (exact averages)
    s = _draw(gen, 1, 4, nd)
    p = tuple(_draw(gen, 0, k_ // 2) for k_ in k)
    # (torch's average pooling rejects an input smaller than the window even where the padding would make up for it)
    size = tuple((max(1, k_ - 2 * p_) if kind.startswith("max") else k_) + _draw(gen, 0, 5) for k_, p_ in zip(k, p))
    return CF.pool(f"sweep-{kind}-{i}", kind, 2, k, size, s=s, p=p, N=2, V=1, x="ties" if i % 2 else None, lowering="sweep", edge="sweep")


@pytest.mark.parametrize("kind", ["conv3d", "convT3d", "convT2d", "convT1d", "conv2d", "conv1d", "maxpool3d", "avgpool3d", "maxpool1d", "avgpool1d"])
def test_sweep_of_random_geometries(kind, standins, monkeypatch):
    gen = torch.Generator().manual_seed(20240 + sorted(CF.NDIM).index(kind))
    ran = served = 0
    for i in range(SWEEP):
        case = (_sweep_case if CF.is_conv(kind) else _sweep_pool)(kind, gen, i)
        monkeypatch.setitem(CF.ALL, case.name, case)
        try:
            CF.out_shape(case)
        except RuntimeError:   # torch itself rejects the module (an empty output, a padding beyond half the window)
            continue
        ran += 1
        module, x, M = CF.on_device(case, "exact", "cpu", F64)
        for rule in CF.rules_of(case):
            got = CF.lower(case, rule, module, M, x)
            if rule == "input" and CF.is_transposed(kind):
                no = CF.declines(case)
                assert (got is None) == no, f"{case.spec}: returned {'None' if got is None else 'a tensor'}"
                if no:
                    continue
                served += 1
            W, xo, Mo = CF.operands(case, "exact")
            fn = CF.input_rule if rule == "input" else CF.weight_rule
            assert_equal(got, fn(case, W, xo, Mo), f"{rule} rule of {case.spec}")
    print(f"{kind}: {ran} of {SWEEP} random geometries ran" + (f", {served} served by the lowering" if CF.is_transposed(kind) else ""))
    assert ran >= 0.6 * SWEEP, f"only {ran} of {SWEEP} draws ran"


# ---- the try / except of the dispatch ---------------------------------------------------------------------------------------
class _AsIfOnDevice(torch.Tensor):
    """A CPU tensor that answers ``is_cuda`` with True: reaches the kernel branch of ``_jac_t_mat_prod`` without a GPU."""
    is_cuda = property(lambda self: True)


@pytest.mark.parametrize("name", ["c2-g3", "c3-g2", "c1-g3"])
def test_unsupported_falls_through_to_the_generic_rule_and_other_errors_propagate(name, monkeypatch):
    from vivit_amd import kernels

    case = CF.ALL[name]
    module, x, M = CF.on_device(case, "exact", "cpu", torch.float32)   # (fp32: the dtype gate; integers, so still exact)
    calls = []

    def refuse(status):
        def fn(*a, **k):
            calls.append(status)
            raise _lib.VivitHipError(f"vivit_conv2d_jac_t_f32: status {status}", status)
        return fn

    generic_rule = ext._generic_jac_t_mat_prod   # (the real one, on the plain tensor: batched autograd knows no subclasses)
    monkeypatch.setattr(ext, "_generic_jac_t_mat_prod", lambda m, M_, x_: generic_rule(m, M_.as_subclass(torch.Tensor), x_))
    monkeypatch.setattr(kernels, "conv2d_jac_t", refuse(_lib.VIVIT_E_UNSUPPORTED))
    got = ext._jac_t_mat_prod(module, M.as_subclass(_AsIfOnDevice), x)
    assert calls == [_lib.VIVIT_E_UNSUPPORTED], "the kernel branch was not reached"
    assert_equal(got.as_subclass(torch.Tensor), CF.reference(name, "input", "exact")[0], name)
    other = next(s for s in (_lib.VIVIT_E_BADARG, _lib.VIVIT_E_LAUNCH) if s != _lib.VIVIT_E_UNSUPPORTED)
    monkeypatch.setattr(kernels, "conv2d_jac_t", refuse(other))
    with pytest.raises(_lib.VivitHipError) as err:
        ext._jac_t_mat_prod(module, M.as_subclass(_AsIfOnDevice), x)
    assert err.value.status == other
