"""tests/ssd_refs.py: the reference rules against fp64 autograd of the reference loop, per sample, and the module's loop (CPU)."""
import pytest
import torch

import ssd_refs as refs
from vivit_amd.backend import SelectiveScanSSD

H, P, S, N, T, V = 4, 3, 5, 2, 6, 2


@pytest.mark.parametrize("G,softplus", [(1, True), (2, False), (4, True)])
def test_reference_rules_are_the_adjoints_of_the_loop(G, softplus):
    torch.manual_seed(G)
    mod = SelectiveScanSSD(H, P, S, G, softplus).double()
    with torch.no_grad():
        mod.dt_bias.copy_(torch.randn(H))
        mod.D.copy_(torch.randn(H))
    x, M = torch.randn(N, T, H * P + H + 2 * G * S, dtype=refs.F64, requires_grad=True), torch.randn(V, N, T, H * P, dtype=refs.F64)
    params = (mod.A_log, mod.D, mod.dt_bias)
    y = refs.scan(x, *params, H, P, S, G, softplus)
    assert torch.allclose(mod.scan_loop(x), y, rtol=1e-12, atol=1e-12) and torch.equal(mod(x), mod.scan_loop(x))
    got = refs.rules(M, x.detach(), *(p.detach() for p in params), H, P, S, G, softplus)
    for v in range(V):
        for n in range(N):
            want = torch.autograd.grad(y[n], (x,) + params, M[v, n], retain_graph=True)
            assert torch.allclose(got[0][v, n], want[0][n], rtol=1e-10, atol=1e-12)
            assert all(torch.allclose(f[v, n], w, rtol=1e-10, atol=1e-12) for f, w in zip(got[1:], want[1:]))
