"""``kernels.symeigvals_batched`` / ``EigvalshComputation(batched_solve=True)`` on the GPU.

The batched solve runs, per problem, the instruction stream of the single solve -- for 193 <= n <= 1280 the persistent
tridiagonalisation (csrc/sytrd_persist.hip) with problem q on XCD q, each with its own arrival gate, counters and exchange
buffers -- and has no reduction across problems.  So the criterion is EQUALITY OF BYTES with
``symeig(G_i, eigenvectors=False)``: anything weaker would hide an exchange buffer or a counter shared between problems.
The fp64 bound is the one tests/test_persistent_gpu.py::test_sytrd_persistent_spectrum uses for this kernel
(5e-6 max|lambda|).  Reference semantics: the eigenvalues ``Tensor.symeig`` returns per group at
vivit/linalg/eigvalsh.py:221; a batched call has no counterpart there.

Inputs of a batch of B: B - 1 seeded symmetric matrices ``M + M^T`` (as test_persistent_gpu.py) and, last, one
rank-deficient PSD Gram matrix ``V V^T`` of rank n // 3; a batch of one is run with each kind.

The knobs are read once per process, hence the child processes for the other routes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch import nn

import vivit_amd
from helpers import FakeModule, golden_factors, load_golden
from symeig_batched_child import batch_inputs
from vivit_amd import kernels
from vivit_amd.backend import backpack, extend
from vivit_amd.backend.extensions import _materialised_closures

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = torch.device("cuda:0")
SIZES = [64, 192, 193, 256, 300, 777, 1024, 1280]
BATCHES = [1, 3, 8, 11]


def singles(mats):
    return torch.stack([kernels.symeig(G, eigenvectors=False)[0] for G in mats])


def assert_same_bytes(W, S, what=""):
    assert W.shape == S.shape and W.dtype == S.dtype
    for i, (a, b) in enumerate(zip(W.cpu().numpy(), S.cpu().numpy())):
        assert a.tobytes() == b.tobytes(), f"{what} problem {i}: max |diff| {np.abs(a - b).max()}"


def check_against_fp64(W, mats):
    for i, (w, G) in enumerate(zip(W.cpu().double().numpy(), mats)):
        ref = np.linalg.eigvalsh(G.cpu().double().numpy())
        err, scale = np.abs(w - ref).max(), np.abs(ref).max()
        print(f"  problem {i}: max |dlambda| / max |lambda| = {err / scale:.3e}")
        assert err <= 5e-6 * scale, (i, err, scale)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("n", SIZES)
def test_batched_equals_single_solves_bit_for_bit(n, B):
    variants = [batch_inputs(n, B, DEV)]
    if B == 1:   # a batch of one with each kind of matrix
        variants.append(batch_inputs(n, 2, DEV)[:1])
    for mats in variants:
        keep = [G.clone() for G in mats]
        W = kernels.symeigvals_batched(mats)
        assert W.shape == (B, n)
        assert all(torch.equal(G, K) for G, K in zip(mats, keep)), "overwrite=False must leave the inputs alone"
        assert_same_bytes(W, singles(mats), f"n={n} B={B}")
        check_against_fp64(W, mats)
        assert_same_bytes(kernels.symeigvals_batched(mats), W, "second identical call")       # determinism
        assert_same_bytes(kernels.symeigvals_batched(torch.stack(mats)), W, "[B, n, n] input")
        assert_same_bytes(kernels.symeigvals_batched([G.clone() for G in mats], overwrite=True), W, "overwrite=True")


@pytest.mark.parametrize("n", [64, 256, 777, 1280])
def test_no_spectrum_is_returned_twice(n):
    """Eight different matrices: a wrong problem -> pointer mapping would hand out one spectrum twice."""
    mats = batch_inputs(n, 8, DEV)
    W = kernels.symeigvals_batched(mats).cpu()
    for i in range(8):
        for j in range(i + 1, 8):
            assert not torch.equal(W[i], W[j]), (i, j)
    assert_same_bytes(W, singles(mats))


@pytest.mark.parametrize("bad", [0, 5, 7])
@pytest.mark.parametrize("n", [64, 256, 1024])
def test_nan_fails_only_its_own_problem(n, bad):
    mats = batch_inputs(n, 8, DEV)
    good = singles(mats)
    mats[bad][n // 2, n // 3] = float("nan")
    infos = []
    W = kernels.symeigvals_batched(mats, info_out=infos)
    info = infos[0].cpu().tolist()
    assert len(infos) == 1 and len(info) == 8
    assert info[bad] == n and all(v == 0 for i, v in enumerate(info) if i != bad), info
    others = [i for i in range(8) if i != bad]
    assert_same_bytes(W[others], good[others])
    with pytest.raises(RuntimeError, match=f"problem {bad}"):
        kernels.symeigvals_batched(mats)


def test_argument_contract():
    a, b = batch_inputs(256, 2, DEV)
    with pytest.raises(ValueError):
        kernels.symeigvals_batched([a, batch_inputs(300, 1, DEV)[0]])
    with pytest.raises(ValueError):
        kernels.symeigvals_batched([a, b[:, :100]])
    with pytest.raises(ValueError):
        kernels.symeigvals_batched([])
    with pytest.raises(RuntimeError):
        kernels.symeigvals_batched([a.cpu(), b.cpu()])
    # rows of a wider buffer (leading dimension > n) and a transposed view
    wide = torch.zeros(256, 300, device=DEV)
    wide[:, :256] = a
    assert_same_bytes(kernels.symeigvals_batched([wide[:, :256], b.T]), singles([a, b.T.contiguous()]))


def test_sizes_above_one_xcd_fall_back_to_single_solves():
    mats = batch_inputs(1300, 2, DEV)
    assert_same_bytes(kernels.symeigvals_batched(mats), singles(mats))


# ---- the other routes -------------------------------------------------------------------------------------------------
def _child(tmp, tag, **env):
    out = tmp / f"batched_{tag}.json"
    subprocess.run([sys.executable, os.path.join(HERE, "symeig_batched_child.py"), str(out)], env=dict(os.environ, **env),
                   check=True, timeout=600)
    return json.loads(out.read_text())


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("batched")
    return {"on": _child(tmp, "on", VIVIT_SYTRD_PERSIST="1"),
            "off": _child(tmp, "off", VIVIT_SYTRD_PERSIST="0"),
            # the first attempt of every arrival gate gives up at once: the retry queued behind it does the work
            "retry": _child(tmp, "retry", VIVIT_SYTRD_PERSIST="1", VIVIT_PERSIST_FAULT="1")}


def test_launch_chain_route_equals_a_loop_of_single_solves(runs):
    for case, row in runs["off"].items():
        assert row["batched"] == row["single"], case
    # (the knob did select another reduction: the blocked launch chain rounds differently)
    assert any(runs["off"][c]["batched"] != runs["on"][c]["batched"] for c in runs["on"])


def test_aborted_first_attempt_is_retried_per_problem(runs):
    for case, row in runs["retry"].items():
        assert row["batched"] == runs["on"][case]["batched"], case
        assert row["batched"] == row["single"], case
    for case, row in runs["on"].items():
        assert row["batched"] == row["single"], case


# ---- public API --------------------------------------------------------------------------------------------------------
def _per_parameter_spectra(model, X, y, batched, mc_samples=0, samples=None):
    comp = vivit_amd.EigvalshComputation(mc_samples=mc_samples, batched_solve=batched)
    groups = [{"params": [p]} for p in model.parameters()]
    model.zero_grad()
    m, lossf = extend(model), extend(nn.CrossEntropyLoss())
    ext = comp.get_extension()
    if samples is not None:
        ext._samples = samples
    loss = lossf(m(X), y)
    with backpack(ext, extension_hook=comp.get_extension_hook(groups)):
        loss.backward()
    out = [comp.get_result(g) for g in groups]
    with pytest.raises(KeyError):
        comp.get_result({"params": []})
    return out


def test_twelve_linear_layers_batched_equals_immediate():
    """12 single-parameter groups, N C = 128 * 10 = 1280: eight in one launch during the pass, four on get_result."""
    torch.manual_seed(0)
    C, N = 10, 128
    layers = []
    for i in range(12):
        layers += [nn.Linear(C, C, bias=False)] + ([nn.Tanh()] if i < 11 else [])
    model = nn.Sequential(*layers).to(DEV)
    X, y = torch.rand(N, C, device=DEV), torch.randint(0, C, (N,), device=DEV)
    plain = _per_parameter_spectra(model, X, y, batched=False)
    batched = _per_parameter_spectra(model, X, y, batched=True)
    assert len(plain) == len(batched) == 12
    for i, (a, b) in enumerate(zip(batched, plain)):
        assert a.shape == (N * C,) and torch.equal(a, b), i
    torch.cuda.synchronize()
    assert any(not torch.equal(plain[0], p) for p in plain[1:])


def test_resnet32_per_parameter_groups_batched_equals_immediate():
    """BASELINE config 4 (ResNet-32, C = 100, SqrtGGN-MC with one sample, n = N = 1024) with one group per parameter."""
    from helpers import resnet32

    N = 1024
    torch.manual_seed(0)
    model = resnet32(100).to(DEV)
    X, y = torch.rand(N, 3, 32, 32, device=DEV), torch.randint(0, 100, (N,), device=DEV)
    with torch.no_grad():
        probs = model(X).softmax(1)
        idx = torch.multinomial(probs, 1, replacement=True, generator=torch.Generator(device=DEV).manual_seed(2))
        samples = torch.nn.functional.one_hot(idx.t(), 100).float()
    plain = _per_parameter_spectra(model, X, y, batched=False, mc_samples=1, samples=samples)
    batched = _per_parameter_spectra(model, X, y, batched=True, mc_samples=1, samples=samples)
    assert len(plain) == len(batched) == len(list(model.parameters())) > 12
    for i, (a, b) in enumerate(zip(batched, plain)):
        assert a.shape == (N,) and torch.equal(a, b), i


def test_golden_mlp_small_per_parameter_groups():
    """The tolerances of tests/test_api_golden.py::test_eigvalsh (reference: rtol 1e-4, atol 5e-6,
    test/linalg/test_eigvalsh.py:60), with the groups going through the queue."""
    g = load_golden("mlp_small")
    V, _ = golden_factors(g, DEV)
    N, N_total = int(g["N"]), int(g["N_total"])
    sub = None if N == N_total else list(range(N))
    params = [torch.nn.Parameter(torch.zeros(*v.shape[2:], device=DEV)) for v in V]
    comp = vivit_amd.EigvalshComputation(subsampling=sub, batched_solve=True)
    for p, v in zip(params, V):
        setattr(p, comp._savefield, _materialised_closures(v))
    groups = [{"params": [p]} for p in params]
    comp.get_extension_hook(groups)(FakeModule(params, N_total))
    for gi, grp in enumerate(groups):
        ref = g[f"eigvalsh_per_param_{gi}"]
        np.testing.assert_allclose(comp.get_result(grp).cpu().numpy(), ref, rtol=1e-4, atol=1e-5 * np.abs(ref).max())
    assert all(not hasattr(p, comp._savefield) for p in params)
