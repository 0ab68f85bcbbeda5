"""kernels.selective_scan_forward / selective_scan_rules against the fp64 references of tests/selective_scan_refs.py under
|got - ref| <= c (T + S + 4) 2^-24 majorant (derivation of c there)."""
import functools

import pytest
import torch

import selective_scan_refs as refs
from vivit_amd import _lib, kernels

pytestmark = pytest.mark.gpu
CHUNK, CHAN, WAVES = kernels.SSCAN_CHUNK, kernels.SSCAN_CHAN, kernels.SSCAN_WAVES
CASES = {   # id -> V, N, T, D, S, softplus, shift of dt
    "one-step": (2, 2, 1, 5, 16, True, 0.0),
    "past-two-chunks": (2, 2, 2 * CHUNK + 3, 5, 16, True, 0.0),
    "two-channel-blocks": (2, 2, CHUNK + 1, CHAN + 3, 16, True, 0.0),
    "S=1": (2, 2, CHUNK + 1, 5, 1, True, 0.0),
    "S=5": (2, 2, CHUNK + 1, 5, 5, True, 0.0),
    "S=32": (2, 2, CHUNK + 1, 5, 32, True, 0.0),
    "S=64": (2, 2, CHUNK + 1, CHAN + 3, 64, True, 0.0),
    "column-split": (2 * WAVES + 1, 3, CHUNK + 1, 5, 16, True, 0.0),
    "strong-decay": (2, 2, 2 * CHUNK + 3, 5, 16, True, 2.0),      # with A_log in [1, 3]: Delta |A| reaches 20 and more
    "no-softplus": (2, 2, CHUNK + 1, 5, 16, False, 0.0),
}


@functools.lru_cache(maxsize=None)
def problem(name):
    """CPU operands ``(M, x, A_log, Dk)`` and ``[(fp64 reference, bound)]`` for y, g, F_A, F_Dk; computed once, not to be modified."""
    V, N, T, D, S, softplus, shift = CASES[name]
    gen = torch.Generator().manual_seed(len(name))
    x, M = torch.randn(N, T, 2 * D + 2 * S, generator=gen), torch.randn(V, N, T, D, generator=gen)
    A_log, Dk = torch.randn(D, S, generator=gen), torch.randn(D, generator=gen)
    if not softplus:
        x[..., D:2 * D] = x[..., D:2 * D].abs() + 0.01
    if shift:
        x[..., D:2 * D] += shift
        A_log = (0.5 * A_log.abs() + 1.0).clamp(max=3.0)
    ops = (x, A_log, Dk)
    want = (refs.scan(*ops, softplus),) + refs.rules(M, *ops, softplus)
    major = (refs.scan(*ops, softplus, majorant=True),) + refs.rules(M, *ops, softplus, majorant=True)
    return (M,) + ops, [(r, refs.bound(m, x, A_log, softplus)) for r, m in zip(want, major)]


def run(name, want=(True, True, True)):
    M, x, A_log, Dk = (t.cuda() for t in problem(name)[0])
    softplus = CASES[name][5]
    return (kernels.selective_scan_forward(x, A_log, Dk, softplus),) + kernels.selective_scan_rules(M, x, A_log, Dk, softplus, want)


@pytest.mark.parametrize("name", list(CASES))
def test_kernels_match_fp64_references(name):
    got = run(name)
    if name == "strong-decay":
        assert refs.constant(*problem(name)[0][1:3]) >= 26.0
    for what, out, (ref, bound) in zip(("y", "g", "F_A", "F_Dk"), got, problem(name)[1]):
        err = (out.cpu().to(refs.F64) - ref).abs()
        print(name, what, "largest share of the bound used:", float((err / bound.clamp_min(1e-300)).max()))
        assert out.shape == ref.shape and bool((err <= bound).all()), what
    if name == "past-two-chunks":   # the same bytes on every run
        assert all(torch.equal(a, b) for a, b in zip(run(name), got))


@pytest.mark.parametrize("off", [0, 1, 2])
@pytest.mark.parametrize("name", ["two-channel-blocks", "S=64"])
def test_want_subsets_keep_the_other_results_bytes(name, off):
    full, want = run(name)[1:], tuple(i != off for i in range(3))
    part = run(name, want)[1:]
    assert part[off] is None and all(torch.equal(a, b) for i, (a, b) in enumerate(zip(part, full)) if i != off)


def test_65_states_are_refused():
    x, A_log, Dk, M = torch.randn(1, 2, 2 * 4 + 130).cuda(), torch.randn(4, 65).cuda(), torch.randn(4).cuda(), torch.randn(1, 1, 2, 4).cuda()
    for call in (lambda: kernels.selective_scan_forward(x, A_log, Dk), lambda: kernels.selective_scan_rules(M, x, A_log, Dk)):
        with pytest.raises(_lib.VivitHipError, match="status -4"):   # VIVIT_E_UNSUPPORTED
            call()
