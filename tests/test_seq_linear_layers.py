"""The Linear-on-sequence closures through the public API: ``EigvalshComputation`` and ``EighComputation`` on a pre-LN encoder block
whose four sequence Linears take ``_linear_seq_weight_closures`` (``SEQ_LINEAR_EXPLICIT_MAX_BYTES`` patched to 0; route A forced
through ``SEQ_LINEAR_KAPPA``, since at these sizes the planner would take route B), against the oracle's dense GGN."""
import numpy as np
import pytest
import torch
from torch import nn

import vivit_amd
from helpers import set_kernel_backend
from oracle import vivit_oracle as oracle
from vivit_amd import kernels
from vivit_amd.backend import ActiveIdentity, MultiheadSelfAttention, Parallel, Slicing, backpack, extend
from vivit_amd.backend import extensions as ext

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E = 8


def make_problem():
    """The model of tests/test_attention_layers.py::make_problem("encoder_mse"), restated: a pre-LN residual encoder block with
    causal attention and class-token pooling; every weight away from symmetric or trivial values."""
    torch.manual_seed(0)
    model = nn.Sequential(
        Parallel(ActiveIdentity(), nn.Sequential(nn.LayerNorm(E), MultiheadSelfAttention(E, 2, causal=True))),
        Parallel(ActiveIdentity(), nn.Sequential(nn.LayerNorm(E), nn.Linear(E, 12), nn.GELU(), nn.Linear(12, E))),
        Slicing((slice(None), 0)), nn.Linear(E, 3))
    X, y = torch.rand(3, 5, E), torch.rand(3, 3)
    g = torch.Generator().manual_seed(1)
    for p in model.parameters():
        p.data.copy_(torch.rand(p.shape, generator=g) * 1.2 - 0.5)
    for m in model.modules():
        if isinstance(m, nn.LayerNorm):
            m.weight.data.add_(1.0)
    return model, X, y, nn.MSELoss(), "mse"


def sequence_linears(model):
    """The Linears that see [N, T, .]: in- and out-projection of the attention, the two of the MLP (not the head)."""
    lin = [m for m in model.modules() if isinstance(m, nn.Linear)]
    assert len(lin) == 5
    return lin[:4]


def run_backward(model, X, y, lossf, extensions, hook=None):
    model, lossf = extend(model), extend(lossf)
    model.zero_grad()
    loss = lossf(model(X), y)
    with backpack(*extensions, extension_hook=hook):
        loss.backward()
    return loss


class Spies:
    def __init__(self, monkeypatch):
        self.reduces, self.seq_factors, self.closures = [], [], []
        real_reduce, real_factor, real_closures = kernels.gram_seq_reduce, ext._param_factor, ext._linear_seq_weight_closures
        monkeypatch.setattr(kernels, "gram_seq_reduce", lambda *a, **k: self.reduces.append(a[6]) or real_reduce(*a, **k))

        def param_factor(module, name, M, x):   # seq_factors: the Linear weights on sequence inputs that go through _param_factor
            if isinstance(module, nn.Linear) and name == "weight" and M.dim() > 3:
                self.seq_factors.append(tuple(M.shape))
            return real_factor(module, name, M, x)

        monkeypatch.setattr(ext, "_param_factor", param_factor)
        monkeypatch.setattr(ext, "_linear_seq_weight_closures", lambda s, z: self.closures.append(tuple(s.shape)) or real_closures(s, z))


def setup(monkeypatch, threshold, subsampling=None):
    set_kernel_backend(None)
    monkeypatch.setattr(ext, "SEQ_LINEAR_KAPPA", 0.0)
    if threshold is not None:
        monkeypatch.setattr(ext, "SEQ_LINEAR_EXPLICIT_MAX_BYTES", threshold)
    spies = Spies(monkeypatch)
    model, X, y, lossf, loss = make_problem()
    ref_model = make_problem()[0].double()
    Xr = X if subsampling is None else X[subsampling]
    ggn = oracle.dense_ggn(ref_model, Xr.double(), loss)
    return spies, model.to(DEV), X.to(DEV), y.to(DEV), lossf, ggn


def test_eigvalsh_and_eigh_end_to_end(monkeypatch):
    spies, model, X, y, lossf, ggn = setup(monkeypatch, 0)
    comp = vivit_amd.EigvalshComputation()
    groups = [{"params": list(model.parameters())}]
    run_backward(model, X, y, lossf, [comp.get_extension()], comp.get_extension_hook(groups))
    w = comp.get_result(groups[0]).cpu().double()
    ref_w = torch.linalg.eigvalsh(ggn)
    k = min(len(w), len(ref_w))
    np.testing.assert_allclose(w[-k:].numpy(), ref_w[-k:].numpy(), rtol=1e-4, atol=5e-6)
    # every sequence Linear went through the new closures and the kernel (T = 5), no Linear weight through the explicit factor
    assert len(spies.closures) == 4 and all(len(s) == 4 and s[2] == 5 for s in spies.closures)
    assert spies.reduces == [5] * 4 and not spies.seq_factors

    spies.reduces.clear(), spies.closures.clear()
    comp = vivit_amd.EighComputation(warn_small_eigvals=0.0)
    crit = lambda evals: [i for i in range(evals.numel()) if evals[i].abs() >= max(1e-4, 1e-3 * float(evals[-1]))]   # noqa: E731
    groups = [{"params": list(model.parameters()), "criterion": crit}]
    run_backward(model, X, y, lossf, [comp.get_extension()], comp.get_extension_hook(groups))
    evals, evecs = comp.get_result(groups[0])
    assert evals.numel() > 0
    Em = torch.cat([e.flatten(1) for e in evecs], 1).cpu().double()
    np.testing.assert_allclose((Em @ Em.T).numpy(), np.eye(Em.shape[0]), atol=2e-4)
    np.testing.assert_allclose((Em @ ggn).numpy(), (evals.cpu().double()[:, None] * Em).numpy(), rtol=1e-3, atol=2e-4)
    assert len(spies.closures) == 4 and spies.reduces == [5] * 4 and not spies.seq_factors


def test_default_threshold_keeps_todays_path(monkeypatch):
    spies, model, X, y, lossf, ggn = setup(monkeypatch, None)
    comp = vivit_amd.EigvalshComputation()
    groups = [{"params": list(model.parameters())}]
    run_backward(model, X, y, lossf, [comp.get_extension()], comp.get_extension_hook(groups))
    w = comp.get_result(groups[0]).cpu().double()
    ref_w = torch.linalg.eigvalsh(ggn)
    k = min(len(w), len(ref_w))
    np.testing.assert_allclose(w[-k:].numpy(), ref_w[-k:].numpy(), rtol=1e-4, atol=5e-6)
    assert not spies.reduces and not spies.closures and len(spies.seq_factors) == 4


def test_subsampling_gives_the_rows_of_the_permuted_batch(monkeypatch):
    sub = [2, 0, 1]
    spies, model, X, y, lossf, _ = setup(monkeypatch, 0)
    ref_model, Xc, _, _, loss = make_problem()
    S = oracle.loss_hessian_sqrt_exact(ref_model(Xc).detach(), loss)
    V_ref = oracle.sqrt_ggn_factors(ref_model, Xc, S, sub)
    extension = vivit_amd.backend.ViViTGGNExact(subsampling=sub)
    run_backward(model, X, y, lossf, [extension])
    names = [n for n, _ in model.named_parameters()]
    seq_weights = {id(m.weight) for m in sequence_linears(model)}
    g = torch.Generator().manual_seed(5)
    seen = 0
    for name, p, v in zip(names, model.parameters(), V_ref):
        if id(p) not in seq_weights:
            continue
        seen += 1
        cl = p.vivit_ggn_exact
        C, N = cl["shape_cn"]
        assert (C, N) == (3, 3)
        v = v.double()
        flat = v.reshape(C * N, -1)
        G = cl["gram_mat"]().view(C * N, C * N)
        np.testing.assert_allclose(G.cpu().double().numpy(), (flat @ flat.T).numpy(), rtol=1e-4, atol=1e-6 * float((flat @ flat.T).abs().max()))
        # an output that was not sub-sampled has the same shape and permuted rows
        unpermuted = flat.view(C, N, -1)[:, [1, 2, 0]].reshape(C * N, -1)
        assert not np.allclose(G.cpu().double().numpy(), (unpermuted @ unpermuted.T).numpy(), rtol=1e-2, atol=0)
        mat = torch.randn(2, C, N, generator=g)
        np.testing.assert_allclose(cl["V_mat_prod"](mat.to(DEV)).cpu().double().numpy(),
                                   torch.einsum("fcn,cnoi->foi", mat.double(), v).numpy(), rtol=1e-4, atol=1e-6 * float(v.abs().max()) * 10)
        np.testing.assert_allclose(cl["factor"]().cpu().double().numpy(), v.numpy(), rtol=1e-4, atol=1e-6)
    assert seen == 4 and len(spies.closures) == 4
