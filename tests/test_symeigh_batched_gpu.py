"""``kernels.symeig_reduce_batched`` (vivit_symeig_reduce_batched_f32 / vivit_symeig_select_batched_f32) on the GPU.

Phase 1 runs, per problem, the instruction stream of ``symeig_reduce`` (persistent tridiagonalisation with problem q on
XCD q, the Sturm multisection kernel with the problem as a grid dimension) on a state block laid out like the single one:
eigenvalues and the state are held to EQUALITY OF BYTES with the single solve -- anything weaker would hide a buffer
shared between problems.  Phase 2 does NOT reproduce the single select bit for bit: the batched back-transformation
applies the Householder reflectors one by one to each selected row (one wavefront per row), the single select uses
compact-WY products on the tile kernels.  Its eigenvectors are therefore held to the fp64 criteria of
tests/test_symeig_select_gpu.py::_check (against ``numpy.linalg.eigh`` of the fp32 matrix in fp64), with no column skipped
by the gap condition, and to equality of bytes across batch compositions.  Reference semantics: ``evecs[:, keep]`` per
group at vivit/linalg/eigh.py:248-253; a batched call has no counterpart there."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from symeig_batched_child import batch_inputs
from vivit_amd import kernels

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = torch.device("cuda:0")
SIZES = [193, 256, 300, 777, 1024, 1280]
BATCHES = [1, 3, 8, 11]


def same_bytes(a, b, what=""):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert a.tobytes() == b.tobytes(), f"{what}: max |diff| {np.abs(a - b).max()}"


def top(n, k=10):
    return list(range(n - k, n))


def check_fp64(G, w, Z, keep):
    """tests/test_symeig_select_gpu.py::_check for one problem; returns the number of columns the gap condition skipped."""
    n = G.shape[0]
    G64 = G.cpu().double().numpy()
    wref, Zref = np.linalg.eigh(G64)
    scale = np.abs(wref).max()
    err = np.abs(w.cpu().double().numpy() - wref).max()
    Zd = Z.cpu().double().numpy()
    assert Zd.shape == (n, len(keep))
    R = np.abs(G64 @ Zd - Zd * wref[keep]).max()
    orth = np.abs(Zd.T @ Zd - np.eye(len(keep))).max() if keep else 0.0
    print(f"  n={n}: dlambda {err / scale:.2e}  residual {R / scale:.2e}  orth {orth:.2e}")
    assert err <= 1e-5 * scale
    assert R <= 3e-5 * scale
    assert orth <= 1e-4
    skipped = 0
    for col, k in enumerate(keep):
        gap = min(abs(wref[k] - wref[k - 1]) if k > 0 else np.inf, abs(wref[k + 1] - wref[k]) if k + 1 < n else np.inf)
        if gap > 1e-4 * scale:
            dev = np.abs(np.abs(Zd[:, col]) - np.abs(Zref[:, k])).max()
            assert dev <= 2e-2 * (1e-4 * scale / gap) + 2e-3, (k, dev, gap / scale)
        else:
            skipped += 1
    return skipped


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("n", SIZES)
def test_reduction_equals_single_bit_for_bit_and_state_interchanges(n, B):
    mats = batch_inputs(n, B, DEV)
    orig = [G.clone() for G in mats]
    keep = top(n)
    bp = kernels.symeig_reduce_batched(mats)
    assert bp.evals.shape == (B, n) and len(bp.plans) == B
    assert all(torch.equal(G, K) for G, K in zip(mats, orig)), "overwrite=False must leave the inputs alone"
    singles = [kernels.symeig_reduce(G) for G in mats]
    for b in range(B):
        same_bytes(bp.evals[b], singles[b].evals, f"evals n={n} B={B} problem {b}")
        # the single select accepts the batched reduction's state: same bytes as the single reduction's
        same_bytes(bp.plans[b].select(keep), singles[b].select(keep), f"state n={n} B={B} problem {b}")
    same_bytes(kernels.symeig_reduce_batched(mats).evals, bp.evals, "second identical call")
    same_bytes(kernels.symeig_reduce_batched(torch.stack(mats)).evals, bp.evals, "[B, n, n] input")
    same_bytes(kernels.symeig_reduce_batched([G.clone() for G in mats], overwrite=True).evals, bp.evals, "overwrite=True")


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("n", SIZES)
def test_batched_select_meets_the_fp64_criteria(n, B):
    mats = batch_inputs(n, B, DEV)
    keep = top(n)
    bp = kernels.symeig_reduce_batched(mats)
    Zs = bp.select([keep] * B)
    assert len(Zs) == B
    skipped = sum(check_fp64(G, bp.evals[b], Zs[b], keep) for b, G in enumerate(mats))
    assert skipped == 0, "every top-10 eigenvalue of these inputs is isolated: the sign-free comparison must cover all"
    again = bp.select([keep] * B)   # a second select from the same reduction: deterministic
    for b in range(B):
        same_bytes(again[b], Zs[b], f"second select, problem {b}")


@pytest.mark.parametrize("n", SIZES)
def test_vectors_do_not_depend_on_batch_composition(n):
    """The block of a matrix is the same bytes in a batch of 1, 3, 8 or 11, at any position, next to ragged selections."""
    mats = batch_inputs(n, 11, DEV)
    ks = [10, 0, 1, 40, 10, 1, 40, 0, 10, 10, 40]
    keeps = [top(n, k) for k in ks]
    ref = [kernels.symeig_reduce_batched([G]).select([keep])[0] for G, keep in zip(mats, keeps)]   # batches of one
    for b, k in enumerate(ks):
        assert ref[b].shape == (n, k)
    for B in (3, 8, 11):
        for rot in (0, 1, B - 1):
            order = [(i + rot) % B for i in range(B)]
            out = kernels.symeig_reduce_batched([mats[i] for i in order]).select([keeps[i] for i in order])
            for pos, i in enumerate(order):
                same_bytes(out[pos], ref[i], f"n={n} B={B} rot={rot} matrix {i}")


@pytest.mark.parametrize("n", [256, 777, 1280])
def test_no_vector_block_is_returned_twice(n):
    mats = batch_inputs(n, 8, DEV)
    Zs = [Z.cpu() for Z in kernels.symeig_reduce_batched(mats).select([top(n)] * 8)]
    for i in range(8):
        for j in range(i + 1, 8):
            assert not torch.equal(Zs[i], Zs[j]), (i, j)


def test_index_rules_and_many_vectors():
    n = 300
    mats = batch_inputs(n, 3, DEV)
    bp = kernels.symeig_reduce_batched(mats)
    keeps = [[n - 3, n - 40, n - 3, -1], [], list(range(n - 280, n))]   # order + repeats + negative | none | > 256: D&C route
    Zs = bp.select(keeps)
    assert [tuple(Z.shape) for Z in Zs] == [(n, 4), (n, 0), (n, 280)]
    same_bytes(Zs[0][:, 0], Zs[0][:, 2], "repeated index")
    one = bp.select([[n - 1], [], []])[0]
    same_bytes(Zs[0][:, 3], one[:, 0], "negative index")
    same_bytes(Zs[2], bp.plans[2].select(keeps[2]), "a selection above 256 goes through the single select")
    with pytest.raises(IndexError):
        bp.select([[n], [], []])
    with pytest.raises(ValueError):
        bp.select([[0]])


@pytest.mark.parametrize("bad", [0, 5, 7])
@pytest.mark.parametrize("n", [256, 1024])
def test_nan_fails_only_its_own_problem(n, bad):
    mats = batch_inputs(n, 8, DEV)
    keep = top(n)
    good = kernels.symeig_reduce_batched(mats)
    goodZ = good.select([keep] * 8)
    mats[bad][n // 2, n // 3] = float("nan")
    infos = []
    bp = kernels.symeig_reduce_batched(mats, info_out=infos)
    info = infos[0].cpu().tolist()
    assert len(infos) == 1 and info[bad] == n and all(v == 0 for i, v in enumerate(info) if i != bad), info
    for b in range(8):
        if b == bad:
            continue
        same_bytes(bp.evals[b], good.evals[b], f"evals of problem {b}")
        same_bytes(bp.plans[b].select(keep), good.plans[b].select(keep), f"state of problem {b}")
    Zs = bp.select([keep if b != bad else [] for b in range(8)])
    for b in range(8):
        if b != bad:
            same_bytes(Zs[b], goodZ[b], f"vectors of problem {b}")
    with pytest.raises(RuntimeError, match=f"problem {bad}"):
        kernels.symeig_reduce_batched(mats)


@pytest.mark.parametrize("n", [64, 192, 1300])
def test_sizes_outside_the_batched_range_loop_over_single_reductions(n):
    mats = batch_inputs(n, 3, DEV)
    keep = top(n)
    bp = kernels.symeig_reduce_batched(mats)
    Zs = bp.select([keep, [], keep])
    for b, G in enumerate(mats):
        single = kernels.symeig_reduce(G)
        same_bytes(bp.evals[b], single.evals, f"problem {b}")
        same_bytes(Zs[b], single.select(keep if b != 1 else []), f"problem {b}")


def test_argument_contract():
    a, b = batch_inputs(256, 2, DEV)
    with pytest.raises(ValueError):
        kernels.symeig_reduce_batched([a, batch_inputs(300, 1, DEV)[0]])
    with pytest.raises(ValueError):
        kernels.symeig_reduce_batched([])
    with pytest.raises(RuntimeError):
        kernels.symeig_reduce_batched([a.cpu(), b.cpu()])
    wide = torch.zeros(256, 300, device=DEV)
    wide[:, :256] = a
    bp = kernels.symeig_reduce_batched([wide[:, :256], b.T])
    same_bytes(bp.evals[0], kernels.symeig_reduce(a).evals)
    same_bytes(bp.evals[1], kernels.symeig_reduce(b.T.contiguous()).evals)


# ---- the other routes -------------------------------------------------------------------------------------------------
def _child(tmp, tag, **env):
    out = tmp / f"eigh_batched_{tag}.json"
    subprocess.run([sys.executable, os.path.join(HERE, "symeigh_batched_child.py"), str(out)], env=dict(os.environ, **env),
                   check=True, timeout=600)
    return json.loads(out.read_text())


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("eigh_batched")
    return {"on": _child(tmp, "on", VIVIT_SYTRD_PERSIST="1"),
            "off": _child(tmp, "off", VIVIT_SYTRD_PERSIST="0"),
            # the first attempt of every arrival gate gives up at once: the retry queued behind it does the work
            "retry": _child(tmp, "retry", VIVIT_SYTRD_PERSIST="1", VIVIT_PERSIST_FAULT="1")}


@pytest.mark.parametrize("route", ["on", "off", "retry"])
def test_every_route_equals_the_single_reduction(runs, route):
    for case, row in runs[route].items():
        assert row["batched"] == row["single"], case
        assert row["state"] == row["single_select"], case
    if route == "retry":
        for case, row in runs[route].items():
            assert row["batched"] == runs["on"][case]["batched"], case
    if route == "off":   # (the knob did select another reduction: the blocked launch chain rounds differently)
        assert any(runs["off"][c]["batched"] != runs["on"][c]["batched"] for c in runs["on"])
