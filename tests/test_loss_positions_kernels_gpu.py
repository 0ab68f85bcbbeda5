"""The per-position cross-entropy factor kernels (csrc/loss_positions.hip) against the fp64 references of
tests/loss_positions_refs.py: both memory layouts, both modes, every body (16-byte and scalar) and route (a wavefront or a workgroup
per row of classes; lanes along the positions), outputs between guard words and pre-filled with NaN.  Tolerances: those
tests/test_jacobians_gpu.py uses for the [N, C] kernel, rtol 1e-4 and atol 1e-6 (with scales 1 / sqrt(N), N <= 2, of order one).
Further down: every route past the first trip of its grid-stride loop, offsets of S past 2^31 elements, and non-finite logits."""
import functools
import math

import numpy as np
import pytest
import torch

import loss_positions_refs as refs
from vivit_amd import _lib, kernels

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAME = "vivit_ce_pos_sqrt_hessian_f32"
LAYOUTS = [pytest.param(0, id="ncl"), pytest.param(1, id="nlc")]
RTOL, ATOL = 1e-4, 1e-6


@functools.lru_cache(maxsize=None)
def logits_of(N, C, L, seed=0):
    """Seeded logical logits [N, C, L] (CPU fp32; shared, never modified)."""
    return torch.randn(N, C, L, generator=torch.Generator().manual_seed(seed + 7 * C + L)) * 3.0


@functools.lru_cache(maxsize=None)
def indices_of(M, N, C, L):
    return torch.randint(0, C, (M, N, L), generator=torch.Generator().manual_seed(M + C + L), dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def exact_ref(N, C, L):
    return refs.ce_exact(logits_of(N, C, L), 1.0 / math.sqrt(N))


@functools.lru_cache(maxsize=None)
def sampled_ref(M, N, C, L):
    return refs.ce_sampled(logits_of(N, C, L), indices_of(M, N, C, L), 1.0 / math.sqrt(M * N))


def to_memory(z, layout, shift=False):
    """Logical [N, C, L] -> a flat device tensor in the memory order of ``layout``; ``shift``: 4 bytes off 16-byte alignment."""
    flat = (z if layout == 0 else z.movedim(1, 2)).contiguous().flatten()
    buf = torch.empty(flat.numel() + 1, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    mem = buf[1:] if shift else buf[:-1]
    mem.copy_(flat)
    return mem


def launch(z, idx, layout, scale, shift=False):
    """Call the entry point on guarded memory; returns (buffer, flat view, S in logical order [V, N, C, L])."""
    N, C, L = z.shape
    V = C * L if idx is None else idx.shape[0]
    mem = to_memory(z, layout, shift)
    idx_dev = None if idx is None else idx.to(DEV).contiguous()
    buf, view = refs.guarded(V * N * C * L, DEV, shift)
    assert (view.data_ptr() % 16 != 0) == shift and (mem.data_ptr() % 16 != 0) == shift
    st = getattr(_lib.load(), NAME)(mem.data_ptr(), None if idx is None else idx_dev.data_ptr(), view.data_ptr(), N, C, L, V, layout,
                                    float(scale), torch.cuda.current_stream(DEV).cuda_stream)
    _lib.check(st, NAME)
    torch.cuda.synchronize()
    S = view.view(V, N, C, L) if layout == 0 else view.view(V, N, L, C).movedim(3, 2)
    return buf, view, S


def close(got, ref):
    np.testing.assert_allclose(got.cpu().double().numpy(), ref.numpy(), rtol=RTOL, atol=ATOL)


def off_block_is_zero(S, C, L):
    """Rows v = c' L + l' of the exact factor are exactly 0.0 at every position l != l'."""
    Sx = S.reshape(C, L, -1, C, L).permute(1, 4, 0, 2, 3)          # [l', l, c', n, c]
    off = ~torch.eye(L, dtype=torch.bool, device=S.device)
    return bool((Sx[off] == 0.0).all())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("C,L", [(1, 1), (1, 3), (5, 1), (5, 3), (5, 65), (70, 3), (257, 2)])
def test_exact_factor(C, L, N, layout):
    buf, view, S = launch(logits_of(N, C, L), None, layout, 1.0 / math.sqrt(N))
    assert refs.guards_intact(buf, view) and not bool(torch.isnan(view).any())
    close(S, exact_ref(N, C, L).reshape(C * L, N, C, L))
    assert off_block_is_zero(S, C, L)


@pytest.mark.parametrize("layout,C,L", [(1, 8, 4), (1, 1028, 1), (0, 8, 4), (0, 6, 8), (0, 4, 260)])
def test_exact_factor_on_the_16_byte_bodies(layout, C, L):
    """Unit-stride extents that are multiples of four on aligned operands: the 16-byte body of each route (C = 1028: a workgroup per
    row of classes; L = 260: 65 groups of four positions, a second workgroup of position lanes).  The factor has (C L)^2 N elements."""
    N = 1
    buf, view, S = launch(logits_of(N, C, L), None, layout, 1.0)
    assert refs.guards_intact(buf, view) and not bool(torch.isnan(view).any())
    close(S, refs.ce_exact(logits_of(N, C, L), 1.0).reshape(C * L, N, C, L))
    assert off_block_is_zero(S, C, L)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("L", [1, 3, 65, 260])
@pytest.mark.parametrize("C", [1, 5, 70, 300, 1027])
def test_sampled_factor(C, L, M, layout):
    N = 2
    buf, view, S = launch(logits_of(N, C, L), indices_of(M, N, C, L), layout, 1.0 / math.sqrt(M * N))
    assert refs.guards_intact(buf, view) and not bool(torch.isnan(view).any())
    close(S, sampled_ref(M, N, C, L))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_sampled_factor_past_the_lds_cap_of_the_flat_kernel(layout):
    """C = 16 001 classes (the [N, C] kernel refuses C > 15 360: it keeps a sample's probabilities in LDS)."""
    N, C, L, M = 1, 16001, 2, 1
    buf, view, S = launch(logits_of(N, C, L), indices_of(M, N, C, L), layout, 1.0)
    assert refs.guards_intact(buf, view) and not bool(torch.isnan(view).any())
    close(S, refs.ce_sampled(logits_of(N, C, L), indices_of(M, N, C, L), 1.0))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mode", ["exact", "sampled"])
def test_operands_off_16_byte_alignment(mode, layout):
    """Extents that would take the 16-byte bodies, on logits and an output 4 bytes off 16-byte alignment: the scalar bodies."""
    N = 2
    C, L, M = (8, 4, None) if mode == "exact" else (300, 260, 3)
    z = logits_of(N, C, L)
    idx = None if mode == "exact" else indices_of(M, N, C, L)
    scale = 1.0 / math.sqrt(N) if mode == "exact" else 1.0 / math.sqrt(M * N)
    buf, view, S = launch(z, idx, layout, scale, shift=True)
    assert refs.guards_intact(buf, view, shift=True) and not bool(torch.isnan(view).any())
    close(S, exact_ref(N, C, L).reshape(C * L, N, C, L) if mode == "exact" else sampled_ref(M, N, C, L))


def edge_logits(kind, N, C, L):
    z = logits_of(N, C, L, seed=3).clone()
    if kind == "dominant":
        z[:, 2, :] = 1e4
    elif kind == "equal":
        z[:] = 0.25
    elif kind == "masked":
        z[:, 1, :] = float("-inf")
    elif kind == "shifted":
        z -= 1e4
    return z


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C,L", [(5, 3), (8, 4), (1028, 4)])
@pytest.mark.parametrize("kind", ["dominant", "equal", "masked", "shifted"])
def test_logit_edges(kind, C, L, layout):
    """One dominant logit at 1e4, all equal, one class at -inf, everything shifted by -1e4 (as
    tests/test_jacobians_gpu.py::test_cross_entropy_factor_logit_edges): finite everywhere; a masked class has exactly zero rows and
    columns."""
    N, M = 2, 2
    z = edge_logits(kind, N, C, L)
    idx = torch.where(indices_of(M, N, C, L) == 1, torch.zeros((), dtype=torch.int32), indices_of(M, N, C, L))   # (never the masked class)
    scale = 1.0 / math.sqrt(M * N)
    buf, view, S = launch(z, idx, layout, scale)
    assert refs.guards_intact(buf, view) and bool(torch.isfinite(view).all())
    close(S, refs.ce_sampled(z, idx, scale))
    if kind == "masked":
        assert bool((S[:, :, 1, :] == 0.0).all())
    if C * L <= 64:
        buf, view, S = launch(z, None, layout, 1.0 / math.sqrt(N))
        assert refs.guards_intact(buf, view) and bool(torch.isfinite(view).all())
        close(S, refs.ce_exact(z, 1.0 / math.sqrt(N)).reshape(C * L, N, C, L))
        assert off_block_is_zero(S, C, L)
        if kind == "masked":
            assert bool((S[:, :, 1, :] == 0.0).all()) and bool((S[L:2 * L] == 0.0).all())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C,L", [(5, 3), (8, 4)])
def test_an_index_outside_the_classes_matches_no_class(C, L, layout):
    N, M = 2, 2
    z = logits_of(N, C, L)
    idx = indices_of(M, N, C, L).clone()
    bad = [(0, 0, 0, -1), (0, 1, L - 1, C), (1, 0, 1, 2 ** 31 - 1), (1, 1, 0, -2 ** 31)]
    for m, n, l, value in bad:
        idx[m, n, l] = value
    buf, view, S = launch(z, idx, layout, 0.5)
    assert refs.guards_intact(buf, view) and bool(torch.isfinite(view).all())
    close(S, refs.ce_sampled(z, idx, 0.5))
    p = z.double().softmax(1)
    for m, n, l, _ in bad:
        close(S[m, n, :, l], p[n, :, l] * 0.5)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mode,C,L", [("exact", 70, 3), ("sampled", 1027, 65), ("sampled", 300, 260)])
def test_a_second_call_gives_the_same_bytes(mode, C, L, layout):
    N, M = 2, 3
    idx = None if mode == "exact" else indices_of(M, N, C, L)
    first = launch(logits_of(N, C, L), idx, layout, 0.5)[1].clone()
    second = launch(logits_of(N, C, L), idx, layout, 0.5)[1]
    assert torch.equal(first, second)


# ---- past the first trip of the grid-stride loops --------------------------------------------------------------------------------------
# Every launch caps its grid at 32 768 workgroups and loops.  The shapes below are the smallest whose LAST trip holds one row (or one
# group of positions) beyond a whole number of full trips: 4 * 32768 + 1 rows on the wavefront route (one busy wavefront beside three
# idle ones), 32768 + 1 rows on the workgroup route, 64 * 32768 + 1 positions or groups of four on the position lanes.  The logits are
# drawn per test and not cached (up to 135 MB); the fp64 references are the vectorised ones of loss_positions_refs, compared on the
# device in chunks with the formula of numpy's assert_allclose.
def fresh_logits(N, C, L):
    return torch.randn(N, C, L, generator=torch.Generator().manual_seed(11 + 7 * C + L)) * 3.0


def fresh_indices(M, N, C, L):
    return torch.randint(0, C, (M, N, L), generator=torch.Generator().manual_seed(13 + M + C + L), dtype=torch.int32)


def close_on_device(view, ref, layout, chunk=1 << 24):
    """|got - ref| <= ATOL + RTOL |ref| (NaN equal to NaN only) for the flat device ``view`` against the CPU fp64 ``ref`` in logical
    order [V, N, C, L], brought into the memory order of ``layout`` and uploaded ``chunk`` elements at a time."""
    flat = (ref if layout == 0 else ref.movedim(2, 3)).reshape(-1)
    assert flat.numel() == view.numel()
    for o in range(0, flat.numel(), chunk):
        r = flat[o:o + chunk].to(DEV)
        g = view[o:o + chunk].double()
        bad = ~(((g - r).abs() <= ATOL + RTOL * r.abs()) | (g.isnan() & r.isnan()))
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            raise AssertionError(f"{int(bad.sum())} of the {r.numel()} elements from flat offset {o} differ from the fp64 reference; the "
                                 f"first, at {o + i}: got {g[i].item()!r}, reference {r[i].item()!r}")


def tail_of(z, idx, S, K):
    """The last K positions of the last sample (the last K samples where L = 1) -- the end of the last trip -- as a problem of its
    own: (logits, indices, the elements of the large launch's S that the small launch computes)."""
    if z.shape[2] >= K:
        return z[-1:, :, -K:], None if idx is None else idx[:, -1:, -K:], S[:, -1:, :, -K:]
    assert z.shape[2] == 1
    return z[-K:], None if idx is None else idx[:, -K:], S[:, -K:]


def second_trip_checks(N, C, L, M, layout, K):
    """M = None: the exact factor.  (1) every element against fp64, none left at the NaN prefill, guards intact; (2) a second call
    gives the same bytes; (3) the end of the last trip has the bytes it gets when launched alone, within a first trip (as
    tests/test_norm_rules_kernels_gpu.py::test_norm_rules_batch_independence)."""
    z = fresh_logits(N, C, L)
    idx = None if M is None else fresh_indices(M, N, C, L)
    scale = 0.5
    buf, view, S = launch(z, idx, layout, scale)
    assert refs.guards_intact(buf, view)
    nans = int(torch.isnan(view).sum())
    assert nans == 0, f"{nans} of {view.numel()} elements are NaN: never written, or computed from stale statistics"
    ref = refs.ce_exact_vec(z, scale).reshape(C * L, N, C, L) if M is None else refs.ce_sampled_vec(z, idx, scale)
    close_on_device(view, ref, layout)
    del ref
    buf2, view2, _ = launch(z, idx, layout, scale)
    assert refs.guards_intact(buf2, view2) and torch.equal(view, view2)
    del buf2, view2
    z_tail, idx_tail, S_tail = tail_of(z, idx, S, K)
    buf3, view3, S_alone = launch(z_tail, idx_tail, layout, scale)
    assert refs.guards_intact(buf3, view3) and torch.equal(S_alone, S_tail)


ROWS_LAYOUTS = [pytest.param(1, 3, id="nlc-3-samples"), pytest.param(0, None, id="ncl-one-position")]


def rows_shape(rows, layout, N):
    """(N, L) with N L = rows that reach the kernel with a row of classes per position: any split under NLC; L = 1 under NCL."""
    if N is None:
        return rows, 1
    assert rows % N == 0
    return N, rows // N


@pytest.mark.parametrize("layout,N", ROWS_LAYOUTS)
@pytest.mark.parametrize("C", [pytest.param(3, id="scalar-body"), pytest.param(4, id="16-byte-body")])
def test_second_trip_wavefront_route_sampled(C, layout, N):
    """131 073 = 4 * 32768 + 1 rows: trips of 131 072 rows, the last with one row in a workgroup whose other wavefronts have none."""
    N, L = rows_shape(131073, layout, N)
    second_trip_checks(N, C, L, 2, layout, K=8)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_second_trip_wavefront_route_exact(layout):
    """The exact factor has (C L)^2 N elements: affordable at L = 1 only, where both layouts are the same memory."""
    second_trip_checks(131073, 3, 1, None, layout, K=8)


@pytest.mark.parametrize("layout,N", ROWS_LAYOUTS)
@pytest.mark.parametrize("C", [pytest.param(1025, id="scalar-body"), pytest.param(1028, id="16-byte-body")])
def test_second_trip_workgroup_route_sampled(C, layout, N):
    """32 769 rows of more than 1024 classes: the one workgroup of the second trip writes ``red[8]`` again.  135 MB each way."""
    N, L = rows_shape(32769, layout, N)
    second_trip_checks(N, C, L, 1, layout, K=3)


@pytest.mark.parametrize("C", [2, 5])
def test_second_trip_position_lanes_scalar_body(C):
    """2 097 153 = 64 * 32768 + 1 positions in three samples of an odd length (one position per lane; samples straddle wavefronts);
    C = 2 leaves two of the four wavefronts of a workgroup without a class, C = 5 gives them 2, 1, 1, 1."""
    second_trip_checks(3, C, 699051, 2, 0, K=5)


def test_second_trip_position_lanes_16_byte_body():
    """2 097 153 groups of four positions."""
    second_trip_checks(1, 2, 8388612, 1, 0, K=8)


# ---- offsets of S past 2^31 elements ------------------------------------------------------------------------------------------------------
def offsets_past_2_31(N, C, L, M, layout):
    """Sampled, S of 2^31 + 65 536 elements (8 GiB) from 65 536 logits: every slice m on the device against
    (p - onehot(idx[m])) scale with p from CPU fp64, none left at the NaN prefill, guards intact."""
    assert M * N * C * L == 2 ** 31 + 65536 and N * C * L == 65536
    free, _ = torch.cuda.mem_get_info()
    if free < 12 << 30:
        pytest.skip(f"{free / 2 ** 30:.1f} GiB of HBM free: the 8 GiB factor, its 2 GiB of indices and the compare need 12")
    try:
        z = logits_of(N, C, L)
        scale = 0.5
        p = z.double().softmax(1)
        p = (p if layout == 0 else p.movedim(1, 2)).contiguous().to(DEV)               # a sample in memory order, fp64
        classes = torch.arange(C, device=DEV, dtype=torch.int32).view((1, 1, C, 1) if layout == 0 else (1, 1, 1, C))
        idx = torch.randint(0, C, (M, N, L), device=DEV, dtype=torch.int32, generator=torch.Generator(device=DEV).manual_seed(M))
        mem = to_memory(z, layout)
        buf, view = refs.guarded(M * N * C * L, DEV)
        st = getattr(_lib.load(), NAME)(mem.data_ptr(), idx.data_ptr(), view.data_ptr(), N, C, L, M, layout, scale,
                                        torch.cuda.current_stream(DEV).cuda_stream)
        _lib.check(st, NAME)
        torch.cuda.synchronize()
        assert refs.guards_intact(buf, view)
        Sm = view.view(M, N, C, L) if layout == 0 else view.view(M, N, L, C)
        step = (1 << 24) // (N * C * L)
        for m0 in range(0, M, step):
            got = Sm[m0:m0 + step].double()
            assert not bool(got.isnan().any()), f"NaN left in the slices from m = {m0}"
            hit = idx[m0:m0 + step].unsqueeze(2 if layout == 0 else 3) == classes
            want = (p.unsqueeze(0) - hit.double()) * scale
            ok = (got - want).abs() <= ATOL + RTOL * want.abs()
            assert bool(ok.all()), f"{int((~ok).sum())} elements of the slices from m = {m0} (flat offset {m0 * N * C * L}) differ"
    finally:
        buf = view = Sm = idx = got = hit = want = ok = None
        torch.cuda.empty_cache()


def test_offsets_past_2_31_wavefront_route():
    """(m rows + row) C passes 2^31 from m = 32 768 on."""
    offsets_past_2_31(64, 1024, 1, 32769, 1)


def test_offsets_past_2_31_position_lanes():
    """((m N + n) C + c) L + l passes 2^31 in the last slice; the indices alone are 2 GiB, (m N + n) L + l up to 2^29."""
    offsets_past_2_31(1, 4, 16384, 32769, 0)


# ---- non-finite logits ------------------------------------------------------------------------------------------------------------------------
# As torch.softmax (and the references): a NaN or +inf at any class, or -inf at all of them, makes every class of THAT position NaN in
# every slice that writes it, and no other position.  A NaN never becomes a lane's running maximum, so where it stands matters to the
# kernel: the first class a lane folds (below 64 / 256 on the scalar rows bodies, below 256 / 1024 on the 16-byte ones, below 4 on
# the position lanes) or a later visit of the lane.
def nonfinite_cases():
    shapes = [   # (layout, C, L, classes of a lane's second visit, id)
        (1, 5, 3, (), "nlc-wavefront-scalar-5x3"), (1, 8, 4, (), "nlc-wavefront-16-byte-8x4"),
        (1, 70, 3, (64,), "nlc-wavefront-scalar-70x3"), (1, 260, 2, (64, 256), "nlc-wavefront-16-byte-260x2"),
        (1, 1027, 2, (256,), "nlc-workgroup-scalar-1027x2"), (1, 1028, 2, (256, 1024), "nlc-workgroup-16-byte-1028x2"),
        (0, 5, 3, (4,), "ncl-lanes-scalar-5x3"), (0, 8, 4, (4,), "ncl-lanes-16-byte-8x4"), (0, 9, 8, (4,), "ncl-lanes-16-byte-9x8"),
        (0, 6, 65, (4,), "ncl-lanes-scalar-6x65"),
        (0, 5, 1, (), "ncl-wavefront-scalar-5x1"), (0, 8, 1, (), "ncl-wavefront-16-byte-8x1"),
        (0, 70, 1, (64,), "ncl-wavefront-scalar-70x1"), (0, 260, 1, (64, 256), "ncl-wavefront-16-byte-260x1"),
        (0, 1027, 1, (256,), "ncl-workgroup-scalar-1027x1"), (0, 1028, 1, (256, 1024), "ncl-workgroup-16-byte-1028x1"),
    ]
    cases = []
    for layout, C, L, second, name in shapes:
        for c in sorted({0, 3, C - 1, *second}):
            cases.append(pytest.param(layout, C, L, "nan", c, id=f"{name}-nan-at-{c}"))
        cases.append(pytest.param(layout, C, L, "plus_inf", 1, id=f"{name}-plus-inf"))
        cases.append(pytest.param(layout, C, L, "all_minus_inf", None, id=f"{name}-all-minus-inf"))
    return cases


def assert_poisons_its_position_only(buf, view, S, ref, rows, n, l):
    """``rows``: the slices that write position l (every other slice holds a structural zero there)."""
    assert refs.guards_intact(buf, view)
    got = S.cpu()
    assert bool(got[rows, n, :, l].isnan().all()), "a class of the poisoned position came out finite"
    assert torch.equal(got.isnan(), ref.isnan()), f"{int(got.isnan().sum())} NaN for {int(ref.isnan().sum())} in the reference"
    assert int(ref.isnan().sum()) == len(rows) * S.shape[2] and bool(torch.isfinite(got[~ref.isnan()]).all())
    close(S, ref)                                                    # (assert_allclose: NaN equal to NaN, the rest within tolerance)


@pytest.mark.parametrize("layout,C,L,kind,c", nonfinite_cases())
def test_a_non_finite_logit_poisons_its_position_only(layout, C, L, kind, c):
    N, M = 2, 2
    n, l = N - 1, min(1, L - 1)                                      # (L = 4, 8: inside a lane's group of four positions)
    z = logits_of(N, C, L, seed=5).clone()
    if kind == "all_minus_inf":
        z[n, :, l] = float("-inf")
    else:
        z[n, c, l] = float("nan") if kind == "nan" else float("inf")
    idx = indices_of(M, N, C, L)
    buf, view, S = launch(z, idx, layout, 0.5)
    assert_poisons_its_position_only(buf, view, S, refs.ce_sampled_vec(z, idx, 0.5), list(range(M)), n, l)
    if C * L <= 64:
        buf, view, S = launch(z, None, layout, 0.5)
        ref = refs.ce_exact_vec(z, 0.5).reshape(C * L, N, C, L)
        assert_poisons_its_position_only(buf, view, S, ref, [cp * L + l for cp in range(C)], n, l)
        assert off_block_is_zero(S, C, L)


@pytest.mark.parametrize("C,c", [(5, 0), (5, 3), (5, 4), (70, 0), (70, 64), (70, 69), (260, 3), (260, 256), (1027, 0), (1027, 256),
                                 (1028, 1024)])
def test_one_position_has_the_nan_mask_of_the_flat_kernel(C, c):
    """L = 1, a NaN at class c of the middle sample: the mask of ``kernels.ce_sqrt_hessian`` on the same logits, which is that whole
    sample and nothing else."""
    N, M = 3, 2
    z = logits_of(N, C, 1).clone()
    z[1, c, 0] = float("nan")
    z = z.to(DEV)
    flat = kernels.ce_sqrt_hessian(z[:, :, 0].contiguous(), 0.5)
    S = kernels.ce_sqrt_hessian_positions(z, 0.5)
    assert bool(flat[:, 1].isnan().all()) and not bool(flat[:, [0, 2]].isnan().any())
    assert torch.equal(S[..., 0].isnan(), flat.isnan())
    idx = indices_of(M, N, C, 1).to(DEV)
    onehot = torch.nn.functional.one_hot(idx[:, :, 0].long(), C).float()
    flat = kernels.ce_sqrt_hessian(z[:, :, 0].contiguous(), 0.5, onehot=onehot)
    S = kernels.ce_sqrt_hessian_positions(z, 0.5, idx=idx)
    assert bool(flat[:, 1].isnan().all()) and not bool(flat[:, [0, 2]].isnan().any())
    assert torch.equal(S[..., 0].isnan(), flat.isnan())


# ---- the wrapper ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 5, 300, 1027])
def test_one_position_equals_the_flat_kernel(C):
    N, M = 3, 2
    z = logits_of(N, C, 1).to(DEV)                                   # [N, C, 1]
    scale = 1.0 / math.sqrt(N)
    flat = kernels.ce_sqrt_hessian(z[:, :, 0].contiguous(), scale)
    S = kernels.ce_sqrt_hessian_positions(z, scale)
    assert S.shape == (C, N, C, 1)
    np.testing.assert_allclose(S[..., 0].cpu().double().numpy(), flat.cpu().double().numpy(), rtol=RTOL, atol=ATOL)
    idx = indices_of(M, N, C, 1).to(DEV)
    onehot = torch.nn.functional.one_hot(idx[:, :, 0].long(), C).float()
    flat = kernels.ce_sqrt_hessian(z[:, :, 0].contiguous(), scale, onehot=onehot)
    S = kernels.ce_sqrt_hessian_positions(z, scale, idx=idx)
    np.testing.assert_allclose(S[..., 0].cpu().double().numpy(), flat.cpu().double().numpy(), rtol=RTOL, atol=ATOL)


def test_wrapper_keeps_the_memory_format_of_the_logits():
    N, C, D, M = 2, 5, (3, 4), 2
    L = math.prod(D)
    z = logits_of(N, C, L)
    idx = indices_of(M, N, C, L)
    ref_s = refs.ce_sampled(z, idx, 0.5).reshape(M, N, C, *D)
    ref_e = refs.ce_exact(z, 0.5).reshape(C * L, N, C, *D)
    idx_dev = idx.to(DEV).view(M, N, *D)
    # contiguous [N, C, H, W]: lanes along the positions, S contiguous
    a = z.view(N, C, *D).to(DEV)
    S = kernels.ce_sqrt_hessian_positions(a, 0.5, idx=idx_dev)
    assert S.shape == (M, N, C, *D) and S.is_contiguous()
    close(S, ref_s)
    S = kernels.ce_sqrt_hessian_positions(a, 0.5)
    assert S.shape == (C * L, N, C, *D) and S.is_contiguous()
    close(S, ref_e)
    # a permuted view of a contiguous [N, H, W, C]: a row of classes per position, S a view of a contiguous [V, N, H, W, C]
    b = z.view(N, C, *D).permute(0, 2, 3, 1).contiguous().to(DEV).permute(0, 3, 1, 2)
    assert not b.is_contiguous()
    S = kernels.ce_sqrt_hessian_positions(b, 0.5, idx=idx_dev)
    assert S.shape == (M, N, C, *D) and S.movedim(2, -1).is_contiguous()
    close(S, ref_s)
    S = kernels.ce_sqrt_hessian_positions(b, 0.5)
    assert S.shape == (C * L, N, C, *D) and S.movedim(2, -1).is_contiguous()
    close(S, ref_e)
    # neither (every other position of a wider tensor): copied, then as the contiguous case
    wide = torch.zeros(N, C, D[0], 2 * D[1], device=DEV)
    wide[..., ::2] = a
    c = wide[..., ::2]
    assert not c.is_contiguous() and not c.movedim(1, -1).is_contiguous()
    S = kernels.ce_sqrt_hessian_positions(c, 0.5, idx=idx_dev)
    assert S.is_contiguous()
    close(S, ref_s)


def test_wrapper_errors():
    z = torch.zeros(2, 5, 3, device=DEV)
    with pytest.raises(ValueError):
        kernels.ce_sqrt_hessian_positions(torch.zeros(2, 5, device=DEV), 1.0)                              # no position dimension
    with pytest.raises(ValueError):
        kernels.ce_sqrt_hessian_positions(torch.zeros(2, 0, 3, device=DEV), 1.0)                           # C < 1
    with pytest.raises(ValueError):
        kernels.ce_sqrt_hessian_positions(z, 1.0, idx=torch.zeros(1, 2, 3, dtype=torch.int64, device=DEV))   # dtype
    with pytest.raises(ValueError):
        kernels.ce_sqrt_hessian_positions(z, 1.0, idx=torch.zeros(1, 2, 4, dtype=torch.int32, device=DEV))   # shape
    with pytest.raises(ValueError):
        kernels.ce_sqrt_hessian_positions(z, 1.0, idx=torch.zeros(2, 3, dtype=torch.int32, device=DEV))      # no M axis
    with pytest.raises(ValueError):
        kernels.ce_sqrt_hessian_positions(z, 1.0, idx=torch.zeros(1, 2, 5, 3, dtype=torch.int32, device=DEV))   # one-hots, not indices
    with pytest.raises(RuntimeError):
        kernels.ce_sqrt_hessian_positions(z.cpu(), 1.0)
