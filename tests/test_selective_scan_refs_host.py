"""tests/selective_scan_refs.py: the reference rules against fp64 autograd of the reference loop, per sample (CPU)."""
import torch

import selective_scan_refs as refs


def test_reference_rules_match_autograd_of_the_loop():
    V, N, T, D, S = 3, 2, 11, 5, 4
    gen = torch.Generator().manual_seed(0)
    x, M = torch.randn(N, T, 2 * D + 2 * S, generator=gen, dtype=refs.F64), torch.randn(V, N, T, D, generator=gen, dtype=refs.F64)
    A_log, Dk = torch.randn(D, S, generator=gen, dtype=refs.F64), torch.randn(D, generator=gen, dtype=refs.F64)
    for softplus in (True, False):
        g, FA, FD = refs.rules(M, x, A_log, Dk, softplus)
        for v in range(V):
            for n in range(N):
                xi, Ai, Di = (t.clone().requires_grad_(True) for t in (x[n:n + 1], A_log, Dk))
                got = torch.autograd.grad(refs.scan(xi, Ai, Di, softplus), (xi, Ai, Di), M[v, n:n + 1])
                for ours, theirs in zip((g[v, n], FA[v, n], FD[v, n]), (got[0][0], got[1], got[2])):
                    assert torch.allclose(ours, theirs, rtol=1e-11, atol=1e-12)
