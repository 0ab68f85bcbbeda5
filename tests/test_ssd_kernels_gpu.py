"""kernels.ssd_forward / ssd_rules against the per-step fp64 references of tests/ssd_refs.py under
|got - ref| <= c (T + S + P + heads per group + 160) 2^-24 majorant (derivation of c there)."""
import functools

import pytest
import torch

import ssd_refs as refs
from vivit_amd import _lib, kernels

pytestmark = pytest.mark.gpu
Q = kernels.SSD_CHUNK
CASES = {   # id -> V, N, T, H, P, S, G, softplus, shift of dt
    "one-step": (2, 2, 1, 3, 16, 16, 1, True, 0.0),
    "past-one-chunk": (2, 2, Q + 3, 3, 16, 64, 1, True, 0.0),
    "past-two-chunks": (3, 2, 2 * Q + 3, 3, 48, 80, 1, True, 0.0),
    "two-groups": (2, 2, Q + 3, 4, 64, 128, 2, True, 0.0),
    "group-per-head": (2, 1, Q + 3, 2, 64, 16, 2, True, 0.0),
    "strong-decay": (2, 2, 2 * Q + 3, 3, 16, 16, 1, True, 2.0),      # with A_log in [1, 3]: Delta |A| passes 20
    "no-softplus": (2, 2, Q + 3, 3, 48, 64, 1, False, 0.0),
}
NAMES = ("y", "g", "F_A", "F_D", "F_dt_bias")


@functools.lru_cache(maxsize=None)
def problem(name):
    """CPU operands ``(M, x, A_log, D, dt_bias)``, the geometry and ``[(fp64 reference, bound)]`` for y, g and the three factors;
    computed once, not to be modified."""
    V, N, T, H, P, S, G, softplus, shift = CASES[name]
    gen = torch.Generator().manual_seed(len(name))
    x, M = torch.randn(N, T, H * P + H + 2 * G * S, generator=gen), torch.randn(V, N, T, H * P, generator=gen)
    A_log, D, bias = torch.randn(H, generator=gen), torch.randn(H, generator=gen), 0.5 * torch.randn(H, generator=gen)
    dt = x[..., H * P:H * P + H]
    if not softplus:
        dt.copy_(dt.abs() + 0.01 - bias.clamp(max=0.0))   # (Delta = dt + dt_bias stays positive)
    if shift:
        dt += shift
        A_log = (0.5 * A_log.abs() + 1.0).clamp(max=3.0)
    ops, geo = (x, A_log, D, bias), (H, P, S, G, softplus)
    want = (refs.scan(*ops, *geo),) + refs.rules(M, *ops, *geo)
    major = (refs.scan(*ops, *geo, majorant=True),) + refs.rules(M, *ops, *geo, majorant=True)
    return (M,) + ops, geo, [(r, refs.bound(m, x, A_log, bias, *geo)) for r, m in zip(want, major)]


def run(name, want=(True, True, True, True)):
    ops, geo, _ = problem(name)
    M, x, A_log, D, bias = (t.cuda() for t in ops)
    return (kernels.ssd_forward(x, A_log, D, bias, *geo),) + kernels.ssd_rules(M, x, A_log, D, bias, *geo, want=want)


@pytest.mark.parametrize("name", list(CASES))
def test_kernels_match_fp64_references(name):
    got = run(name)
    ops, geo, checks = problem(name)
    if name == "strong-decay":
        assert refs.constant(ops[1], ops[2], ops[4], *geo) >= 22.0
    for what, out, (ref, bound) in zip(NAMES, got, checks):
        err = (out.cpu().to(refs.F64) - ref).abs()
        print(name, what, "largest share of the bound used:", float((err / bound.clamp_min(1e-300)).max()))
        assert out.shape == ref.shape and bool((err <= bound).all()), what
    if name == "past-two-chunks":   # the same bytes on every run
        assert all(torch.equal(a, b) for a, b in zip(run(name), got))


@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_want_subsets_keep_the_other_results_bytes(off):
    full, want = run("two-groups")[1:], tuple(i != off for i in range(4))
    part = run("two-groups", want)[1:]
    assert part[off] is None and all(torch.equal(a, b) for i, (a, b) in enumerate(zip(part, full)) if i != off)
    alone = run("two-groups", tuple(i == off for i in range(4)))[1:]
    assert torch.equal(alone[off], full[off])


@pytest.mark.parametrize("P,S", [(4, 129), (65, 16)])
def test_sizes_beyond_the_variants_are_refused(P, S):
    x, vec, M = torch.randn(1, 2, 2 * P + 2 + 2 * S).cuda(), torch.randn(2).cuda(), torch.randn(1, 1, 2, 2 * P).cuda()
    for call in (lambda: kernels.ssd_forward(x, vec, vec, vec, 2, P, S), lambda: kernels.ssd_rules(M, x, vec, vec, vec, 2, P, S)):
        with pytest.raises(_lib.VivitHipError, match="status -4"):   # VIVIT_E_UNSUPPORTED
            call()
