"""The kernels of the weighted cross-entropy factors against the fp64 references of tests/loss_weighted_refs.py:
``vivit_ce_target_scales_f32`` (the scale of a position from its target) and the two factor entry points that take a scale per
position, ``vivit_ce_pos_sqrt_hessian_w_f32`` (both layouts, both modes, every body and route of csrc/loss_positions.hip) and
``vivit_ce_sqrt_hessian_w_f32`` (the [N, C] kernel of csrc/jacobians.hip).  Outputs lie between guard words and are pre-filled with NaN.

Tolerances.  Factors: the project's own for these kernels, rtol 1e-4 and atol 1e-6 (tests/test_loss_positions_kernels_gpu.py).
Scales: 2^-22 relative to the fp64 reference -- one fp32 rounding (2^-24) plus the difference between the fp64 sum of the kernel
(partials of 256 workgroups, added in index order) and torch's, which is orders of magnitude below it; without class weights every sum
is an exact integer and the result must be the very float ``float32(1 / sqrt(mult count))``."""
import functools
import math

import numpy as np
import pytest
import torch

import loss_positions_refs as base
import loss_weighted_refs as refs
from vivit_amd import _lib, kernels

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
POS, POS_W, FLAT, FLAT_W, SCALES = ("vivit_ce_pos_sqrt_hessian_f32", "vivit_ce_pos_sqrt_hessian_w_f32", "vivit_ce_sqrt_hessian_f32",
                                    "vivit_ce_sqrt_hessian_w_f32", "vivit_ce_target_scales_f32")
RTOL, ATOL = 1e-4, 1e-6
IGNORE = -100


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


# ---- the scales kernel ------------------------------------------------------------------------------------------------------------------
SC = 7                                                               # classes of the scales tests
PATTERNS = ["none", "all", "alternating", "first", "last", "out_of_range"]


@functools.lru_cache(maxsize=None)
def targets_of(R, pattern):
    t = torch.randint(0, SC, (R,), generator=torch.Generator().manual_seed(R))
    if pattern == "all":
        t[:] = IGNORE
    elif pattern == "alternating":
        t[1::2] = IGNORE
    elif pattern == "first":
        t[0] = IGNORE
    elif pattern == "last":
        t[-1] = IGNORE
    elif pattern == "out_of_range":
        t[R // 2] = SC + 3
        t[0] = -7 if R > 1 else t[0]
    return t


@functools.lru_cache(maxsize=None)
def class_weights(C=SC):
    return torch.rand(C, generator=torch.Generator().manual_seed(C)) + 0.25


def launch_scales(t, C, w, eps, mean, mult, ignore_index=IGNORE):
    R = t.numel()
    lib = _lib.load()
    t_dev = t.to(DEV)
    w_dev = None if w is None else w.to(DEV)
    buf, view = refs.guarded(R, DEV)
    nbytes = lib.vivit_ce_target_scales_f32_workspace_bytes(R, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    st = getattr(lib, SCALES)(t_dev.data_ptr(), None if w is None else w_dev.data_ptr(), view.data_ptr(), R, C, ignore_index, eps,
                              1 if mean else 0, mult, ws.data_ptr(), nbytes, stream())
    _lib.check(st, SCALES)
    torch.cuda.synchronize()
    assert refs.guards_intact(buf, view)
    return view


def check_scales(t, C, w, eps, mean, mult, ignore_index=IGNORE):
    got = launch_scales(t, C, w, eps, mean, mult, ignore_index)
    again = launch_scales(t, C, w, eps, mean, mult, ignore_index)
    assert torch.equal(got, again) or (bool(torch.equal(got.isnan(), again.isnan())) and torch.equal(got.nan_to_num(), again.nan_to_num()))
    ref = refs.target_scales(t, C, w, ignore_index, eps, mean, mult)
    g = got.cpu().double()
    assert not bool(g.isnan().any()), "a scale was left at the NaN prefill"
    bad = (g - ref).abs() > 2.0 ** -22 * ref.abs()
    assert not bool(bad.any()), f"{int(bad.sum())} of {t.numel()} scales differ: first at {int(bad.nonzero()[0])}"
    counted = refs.counted_positions(t, C, ignore_index)
    assert bool((g[~counted] == 0).all())
    if w is None:                                                    # bit for bit the float the unweighted entry points are handed
        count = int(counted.sum()) if mean else 1
        want = np.float32(1.0 / math.sqrt(mult * count)) if count else np.float32(0)
        assert bool((got.cpu()[counted] == float(want)).all()), (got.cpu()[counted][:4], want)
    return got


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("R", [1, 5, 257, 65541])
def test_target_scales(R, pattern):
    """65 541 rows: the 256 workgroups of the partial sums take 1024 rows a trip, so 5 rows lie in a second trip of the first one."""
    t = targets_of(R, pattern)
    for w in (None, class_weights()):
        for eps in (0.0, 0.1):
            for mean in (True, False):
                for mult in (1, 3):
                    check_scales(t, SC, w, eps, mean, mult)


def test_target_scales_past_the_first_trip_of_the_rows_kernel():
    """32 768 * 256 + 5 rows: the kernel that writes the scales loops too."""
    R = 32768 * 256 + 5
    t = torch.randint(0, SC, (R,), generator=torch.Generator().manual_seed(3))
    t[1::2] = IGNORE
    t[-5:] = torch.tensor([2, IGNORE, 0, SC, 6])
    got = check_scales(t, SC, class_weights(), 0.1, True, 3)
    assert float(got[-5]) > 0 and float(got[-4]) == 0 and float(got[-2]) == 0 and float(got[-1]) > 0
    check_scales(t, SC, None, 0.0, True, 1)


def test_target_scales_with_an_ignore_index_among_the_classes():
    """``ignore_index=2`` with 7 classes, and 255 with 21 (segmentation): a class number can be the ignored one."""
    t = targets_of(257, "none")
    got = check_scales(t, SC, class_weights(), 0.1, True, 1, ignore_index=2)
    assert bool((got.cpu()[t == 2] == 0).all()) and int((t == 2).sum()) > 0
    t = torch.randint(0, 21, (300,), generator=torch.Generator().manual_seed(5))
    t[::7] = 255
    check_scales(t, 21, class_weights(21), 0.0, True, 1, ignore_index=255)


def test_target_scales_edge_decisions():
    """A negative class weight: NaN at its rows only (sum), the rest untouched.  Everything ignored: zeros, not 0 / 0."""
    t = torch.tensor([0, 1, 2, IGNORE, 1])
    w = torch.tensor([1.0, -2.0, 4.0, 1.0, 1.0, 1.0, 1.0])
    got = launch_scales(t, SC, w, 0.0, False, 1).cpu()
    assert got[0] == 1.0 and got[2] == 2.0 and got[3] == 0.0 and bool(got[[1, 4]].isnan().all())
    got = launch_scales(torch.full((300,), IGNORE), SC, class_weights(), 0.1, True, 3)
    assert bool((got == 0).all())


def test_target_scales_wrapper():
    t = targets_of(257, "alternating").view(1, 257)
    got = kernels.ce_target_scales(t.to(DEV), SC, weight=class_weights().to(DEV), label_smoothing=0.1, mean=True, mult=3)
    assert got.shape == t.shape and got.dtype == torch.float32
    assert torch.equal(got.flatten(), launch_scales(t.flatten(), SC, class_weights(), 0.1, True, 3))
    with pytest.raises(RuntimeError):
        kernels.ce_target_scales(t, SC)                                                # a CPU tensor
    with pytest.raises(RuntimeError):
        kernels.ce_target_scales(t.to(DEV).int(), SC)                                  # not int64
    with pytest.raises(ValueError):
        kernels.ce_target_scales(t.to(DEV), SC, weight=torch.ones(SC + 1, device=DEV))
    with pytest.raises(ValueError):
        kernels.ce_target_scales(t.to(DEV), SC, mult=0)


# ---- the factor kernels -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def logits_of(N, C, L, seed=0):
    """Seeded logical logits [N, C, L] (CPU fp32; shared, never modified)."""
    return torch.randn(N, C, L, generator=torch.Generator().manual_seed(seed + 7 * C + L)) * 3.0


@functools.lru_cache(maxsize=None)
def indices_of(M, N, C, L):
    return torch.randint(0, C, (M, N, L), generator=torch.Generator().manual_seed(M + C + L), dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def scales_of(N, L):
    """Seeded scales [N, L] in [0.5, 1.5) with zeros at every position r = n L + l with r % 3 == 1: among the first four positions
    (one lane of the 16-byte position-lanes body) the second is zero and the other three are not."""
    s = torch.rand(N, L, generator=torch.Generator().manual_seed(N + L)) + 0.5
    s.view(-1)[1::3] = 0.0
    return s


def to_memory(z, layout, shift=False):
    """Logical [N, C, L] -> a flat device tensor in the memory order of ``layout``; ``shift``: 4 bytes off 16-byte alignment."""
    flat = (z if layout == 0 else z.movedim(1, 2)).contiguous().flatten()
    buf = torch.empty(flat.numel() + 1, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    mem = buf[1:] if shift else buf[:-1]
    mem.copy_(flat)
    return mem


def shifted(t, shift):
    """A device copy of the flat tensor ``t``, 4 bytes off 16-byte alignment if ``shift``."""
    buf = torch.empty(t.numel() + 5, dtype=t.dtype, device=DEV)
    out = buf[1:1 + t.numel()] if shift else buf[:t.numel()]
    out.copy_(t.flatten())
    assert (out.data_ptr() % 16 != 0) == shift
    return out


def launch(z, idx, layout, scale, shift=False):
    """Logical z [N, C, L], idx [M, N, L] or None.  ``scale`` a tensor [N, L]: the _w entry point; a float: the unweighted one.
    Returns (flat view, S in logical order [V, N, C, L]); the guard words are checked here."""
    N, C, L = z.shape
    V = C * L if idx is None else idx.shape[0]
    mem = to_memory(z, layout, shift)
    idx_dev = None if idx is None else shifted(idx, shift)
    buf, view = refs.guarded(V * N * C * L, DEV, shift)
    lib = _lib.load()
    ip = None if idx is None else idx_dev.data_ptr()
    if isinstance(scale, torch.Tensor):
        s_dev = shifted(scale.float(), shift)
        st = getattr(lib, POS_W)(mem.data_ptr(), ip, s_dev.data_ptr(), view.data_ptr(), N, C, L, V, layout, stream())
    else:
        st = getattr(lib, POS)(mem.data_ptr(), ip, view.data_ptr(), N, C, L, V, layout, float(scale), stream())
    _lib.check(st, POS_W)
    torch.cuda.synchronize()
    assert refs.guards_intact(buf, view, shift)
    S = view.view(V, N, C, L) if layout == 0 else view.view(V, N, L, C).movedim(3, 2)
    return view, S


def launch_flat(z, onehot, scale, shift=False):
    """z [N, C], onehot [M, N, C] or None; ``scale`` a tensor [N] (the _w entry point) or a float."""
    N, C = z.shape
    V = C if onehot is None else onehot.shape[0]
    mem = shifted(z, shift)
    oh = None if onehot is None else shifted(onehot, shift)
    buf, view = refs.guarded(V * N * C, DEV, shift)
    lib = _lib.load()
    op = None if onehot is None else oh.data_ptr()
    if isinstance(scale, torch.Tensor):
        s_dev = shifted(scale.float(), shift)
        st = getattr(lib, FLAT_W)(mem.data_ptr(), op, s_dev.data_ptr(), view.data_ptr(), N, C, V, stream())
    else:
        st = getattr(lib, FLAT)(mem.data_ptr(), op, view.data_ptr(), N, C, V, float(scale), stream())
    _lib.check(st, FLAT_W)
    torch.cuda.synchronize()
    assert refs.guards_intact(buf, view, shift)
    return view, view.view(V, N, C)


def weighted_ref(z, idx, s):
    """fp64: the unweighted factor (scale 1) times s [N, L] at every position, zeros by assignment where s == 0."""
    S = base.ce_exact_vec(z, 1.0) if idx is None else base.ce_sampled_vec(z, idx, 1.0)
    return refs.scale_factor(S, s.double() ** 2)


def close(got, ref):
    g = got.double()
    r = ref.to(DEV)
    bad = ~(((g - r).abs() <= ATOL + RTOL * r.abs()) | (g.isnan() & r.isnan()))
    if bool(bad.any()):
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{int(bad.sum())} of {r.numel()} elements differ from the fp64 reference; the first, at {i}: got "
                             f"{g[tuple(i)].item()!r}, reference {r[tuple(i)].item()!r}")


def zero_positions_are_zero(S, s):
    dead = (s == 0).to(S.device)                                     # [N, L]
    return bool((S.movedim(2, -1)[:, dead] == 0).all())


def modes():
    return [pytest.param(None, id="exact"), pytest.param(1, id="sampled-1"), pytest.param(3, id="sampled-3")]


SHIFTS = [pytest.param(False, id="aligned"), pytest.param(True, id="shifted")]
N2 = 2


def check_positions(C, L, M, layout, shift):
    z, s = logits_of(N2, C, L), scales_of(N2, L)
    idx = None if M is None else indices_of(M, N2, C, L)
    view, S = launch(z, idx, layout, s, shift)
    assert not bool(torch.isnan(view).any())
    close(S, weighted_ref(z, idx, s))
    assert zero_positions_are_zero(S, s)
    # a constant scale array: the bytes of the unweighted entry point
    const = torch.full((N2, L), 0.37)
    assert torch.equal(launch(z, idx, layout, const, shift)[0], launch(z, idx, layout, 0.37, shift)[0])


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("M", modes())
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("C", [5, 70, 1027, 1028])
def test_rows_of_classes(C, L, M, shift):
    """NLC: a wavefront per row (C <= 1024) or a workgroup (C = 1027 scalar, 1028 the 16-byte body when aligned)."""
    check_positions(C, L, M, 1, shift)


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("M", modes())
@pytest.mark.parametrize("C", [5, 6])
@pytest.mark.parametrize("L", [3, 65, 260])
def test_position_lanes(L, C, M, shift):
    """NCL: one position per lane, or four (L = 260 on aligned operands; the first group of four holds one zero scale and three
    others); L = 65 and 260 need a second workgroup / a second wavefront's worth of lanes."""
    check_positions(C, L, M, 0, shift)


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("M", modes())
@pytest.mark.parametrize("C", [1, 5, 300])
@pytest.mark.parametrize("N", [1, 3, 65])
def test_flat_kernel(N, C, M, shift):
    z = logits_of(N, C, 1)[:, :, 0]
    s = scales_of(N, 1)
    idx = None if M is None else indices_of(M, N, C, 1)
    onehot = None if M is None else torch.nn.functional.one_hot(idx[:, :, 0].long(), C).float()
    view, S = launch_flat(z, onehot, s[:, 0], shift)
    assert not bool(torch.isnan(view).any())
    close(S, weighted_ref(z.unsqueeze(-1), idx, s)[..., 0])
    assert bool((S[:, (s[:, 0] == 0).to(DEV)] == 0).all())
    const = torch.full((N,), 0.37)
    assert torch.equal(launch_flat(z, onehot, const, shift)[0], launch_flat(z, onehot, 0.37, shift)[0])


# ---- garbage under zero scales; NaN under counted ones ----------------------------------------------------------------------------------
ROUTES = [  # (layout, C, L): every body of every route
    pytest.param(1, 5, 3, id="nlc-wavefront-scalar"), pytest.param(1, 8, 4, id="nlc-wavefront-16-byte"),
    pytest.param(1, 1027, 2, id="nlc-workgroup-scalar"), pytest.param(1, 1028, 2, id="nlc-workgroup-16-byte"),
    pytest.param(0, 5, 3, id="ncl-lanes-scalar"), pytest.param(0, 6, 8, id="ncl-lanes-16-byte"), pytest.param(0, 5, 65, id="ncl-lanes-scalar-65"),
]
GARBAGE = ["nan", "plus_inf", "all_minus_inf"]


def poisoned(z, kind, n, l):
    z = z.clone()
    if kind == "all_minus_inf":
        z[n, :, l] = float("-inf")
    else:
        z[n, min(3, z.shape[1] - 1), l] = float("nan") if kind == "nan" else float("inf")
    return z


@pytest.mark.parametrize("kind", GARBAGE)
@pytest.mark.parametrize("layout,C,L", ROUTES)
def test_garbage_under_a_zero_scale_is_not_seen(layout, C, L, kind):
    """Position r = 1 (n = 0, l = 1) has scale zero -- inside the first group of four on the 16-byte position lanes: whatever its
    logits hold, the factor has the bytes it has on clean logits: zeros there, the neighbours untouched."""
    z, s = logits_of(N2, C, L), scales_of(N2, L)
    assert s.view(-1)[:3].tolist()[1] == 0.0 and float(s.view(-1)[0]) != 0.0 and float(s.view(-1)[2]) != 0.0
    for M in (None, 2):
        if M is None and C * L > 64:
            continue                                                 # (the exact factor of the long rows: test_rows_of_classes)
        idx = None if M is None else indices_of(M, N2, C, L)
        clean = launch(z, idx, layout, s)[0]
        view, S = launch(poisoned(z, kind, 0, 1), idx, layout, s)
        assert torch.equal(view, clean) and bool(torch.isfinite(view).all()) and zero_positions_are_zero(S, s)


@pytest.mark.parametrize("kind", GARBAGE)
@pytest.mark.parametrize("layout,C,L", ROUTES)
def test_a_non_finite_logit_under_a_counted_position_poisons_it_as_before(layout, C, L, kind):
    """Position r = 2 (beside the zero-scale r = 1) is counted: every class of it is NaN in every slice that writes it, nothing else
    is (the rule of the unweighted entry point), and the zero-scale positions beside it stay zero."""
    z, s = poisoned(logits_of(N2, C, L), kind, *divmod(2, L)), scales_of(N2, L)
    assert float(s.view(-1)[2]) != 0.0
    for M in (None, 2):
        if M is None and C * L > 64:
            continue
        idx = None if M is None else indices_of(M, N2, C, L)
        view, S = launch(z, idx, layout, s)
        ref = weighted_ref(z, idx, s)
        assert torch.equal(S.isnan().cpu(), ref.isnan()) and int(ref.isnan().sum()) == (C if M is None else M) * C
        close(S, ref)
        assert zero_positions_are_zero(S, s)


@pytest.mark.parametrize("kind", GARBAGE)
def test_flat_kernel_garbage_and_nan(kind):
    N, C = 5, 70
    z, s = logits_of(N, C, 1), scales_of(N, 1)
    assert float(s[1, 0]) == 0.0 and float(s[2, 0]) != 0.0
    idx = indices_of(2, N, C, 1)
    onehot = torch.nn.functional.one_hot(idx[:, :, 0].long(), C).float()
    for oh, k in ((None, None), (onehot, idx)):
        clean = launch_flat(z[:, :, 0], oh, s[:, 0])[0]
        assert torch.equal(launch_flat(poisoned(z, kind, 1, 0)[:, :, 0], oh, s[:, 0])[0], clean)
        zp = poisoned(z, kind, 2, 0)
        view, S = launch_flat(zp[:, :, 0], oh, s[:, 0])
        ref = weighted_ref(zp, k, s)[..., 0]
        assert torch.equal(S.isnan().cpu(), ref.isnan()) and bool(S[:, 2].isnan().all())
        close(S, ref)


# ---- zero-scale rows in a later trip of the grid-stride loops ---------------------------------------------------------------------------
# Every launch caps its grid at 32 768 workgroups and loops (tests/test_loss_positions_kernels_gpu.py holds the unweighted entry point
# to fp64 at these very shapes).  Here: the scale array is one constant except for zeros at a few positions of the first trip and at
# the last positions of the last trip, whose logits are NaN; every element must have the bytes of the unweighted entry point on clean
# logits, and zero where the scale is zero -- compared on the device.  The [N, C] kernel has one workgroup per sample and no loop.
def later_trip_check(N, C, L, layout):
    M = 1
    z = torch.randn(N, C, L, generator=torch.Generator().manual_seed(11 + C)) * 3.0
    idx = torch.randint(0, C, (M, N, L), generator=torch.Generator().manual_seed(13 + C), dtype=torch.int32)
    s = torch.full((N, L), 0.37)
    dead = torch.zeros(N * L, dtype=torch.bool)
    dead[[1, 6]] = True
    dead[-3:] = True
    dead[-6] = True
    s.view(-1)[dead] = 0.0
    plain, S_plain = launch(z, idx, layout, 0.37)
    rows = z.movedim(1, 2).contiguous()                              # [N, L, C]
    rows.view(N * L, C)[dead] = float("nan")
    view, S = launch(rows.movedim(2, 1), idx, layout, s)
    assert not bool(torch.isnan(view).any())
    dead_dev = dead.view(N, L).to(DEV)
    want = torch.where(dead_dev.view(1, N, 1, L), torch.zeros((), device=DEV), S_plain)
    assert torch.equal(S, want)


@pytest.mark.parametrize("C", [pytest.param(3, id="scalar-body"), pytest.param(4, id="16-byte-body")])
def test_later_trip_wavefront_route(C):
    later_trip_check(3, C, 131073 // 3, 1)                           # 4 * 32768 + 1 rows


@pytest.mark.parametrize("C", [pytest.param(1025, id="scalar-body"), pytest.param(1028, id="16-byte-body")])
def test_later_trip_workgroup_route(C):
    later_trip_check(3, C, 32769 // 3, 1)                            # 32768 + 1 rows


def test_later_trip_position_lanes_scalar_body():
    later_trip_check(3, 2, 699051, 0)                                # 64 * 32768 + 1 positions


def test_later_trip_position_lanes_16_byte_body():
    later_trip_check(1, 2, 8388612, 0)                               # 64 * 32768 + 1 groups of four


# ---- the wrappers -----------------------------------------------------------------------------------------------------------------------
def test_wrappers_keep_the_memory_format_and_refuse_wrong_shapes():
    N, C, D, M = 2, 5, (3, 4), 2
    L = math.prod(D)
    z, s, idx = logits_of(N, C, L), scales_of(N, L), indices_of(M, N, C, L)
    ref_s, ref_e = weighted_ref(z, idx, s).reshape(M, N, C, *D), weighted_ref(z, None, s).reshape(C * L, N, C, *D)
    s_dev, idx_dev = s.view(N, *D).to(DEV), idx.to(DEV).view(M, N, *D)
    a = z.view(N, C, *D).to(DEV)
    b = z.view(N, C, *D).permute(0, 2, 3, 1).contiguous().to(DEV).permute(0, 3, 1, 2)
    for x in (a, b):
        S = kernels.ce_sqrt_hessian_positions_w(x, s_dev, idx=idx_dev)
        assert S.shape == (M, N, C, *D) and (S if x is a else S.movedim(2, -1)).is_contiguous()
        close(S, ref_s)
        S = kernels.ce_sqrt_hessian_positions_w(x, s_dev)
        assert S.shape == (C * L, N, C, *D) and (S if x is a else S.movedim(2, -1)).is_contiguous()
        close(S, ref_e)
    with pytest.raises(ValueError):
        kernels.ce_sqrt_hessian_positions_w(a, s_dev.flatten())
    with pytest.raises(ValueError):
        kernels.ce_sqrt_hessian_positions_w(a[:, :, 0, 0], s_dev)
    with pytest.raises(RuntimeError):
        kernels.ce_sqrt_hessian_positions_w(a, s_dev.cpu())
    with pytest.raises(ValueError):
        kernels.ce_sqrt_hessian_w(a[:, :, 0, 0].contiguous(), torch.ones(N + 1, device=DEV))
    flat = kernels.ce_sqrt_hessian_w(a[:, :, 0, 0].contiguous(), torch.full((N,), 0.5, device=DEV))
    assert torch.equal(flat, kernels.ce_sqrt_hessian(a[:, :, 0, 0].contiguous(), 0.5))
