"""The per-position cross-entropy factor kernels (csrc/loss_positions.hip) against the fp64 references of
tests/loss_positions_refs.py: both memory layouts, both modes, every body (16-byte and scalar) and route (a wavefront or a workgroup
per row of classes; lanes along the positions), outputs between guard words and pre-filled with NaN.  Tolerances: those
tests/test_jacobians_gpu.py uses for the [N, C] kernel, rtol 1e-4 and atol 1e-6 (with scales 1 / sqrt(N), N <= 2, of order one)."""
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
