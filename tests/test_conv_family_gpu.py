"""The lowerings of the convolution family (vivit_amd/backend/extensions.py) on the REAL kernels, fp32 on the device, against
the fp64 CPU references of tests/conv_family_refs.py: Conv1d, grouped Conv2d, Conv3d, ConvTranspose1d/2d/3d, Max/AvgPool1d and
Max/AvgPool3d at the edge geometries of the case list there (empty and single-slice depth taps, windows that cross a slice of
the stack, output paddings that leave OH / OW below the floor formula, batches of N OD and V N rows, padding (0, pw), group
slices, the matrix-pipe kernels reached through the stack).  tests/test_conv_family_refs_host.py pins every case to the
planner route it is labelled with.

Every (case, rule, family) runs through the lowering function and through the dispatch (``_jac_t_mat_prod`` /
``_param_factor``): exact family bit-equal to fp64, generic family within the derived bound (worst error / bound printed),
two runs of the kernels bit-equal, entries without a single non-zero term exactly zero.  Cases the lowering serves run the dispatch with the
torch rules patched to raise; cases it declines must come back right through the generic rule.  ``mfma``-labelled cases run
again in a child with VIVIT_CONV_MFMA=0."""
import os
import subprocess
import sys

import pytest
import torch

import conv_family_refs as CF
from vivit_amd import _lib
from vivit_amd.backend import extensions as ext

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = torch.device("cuda:0")


def check(got, name, rule, fam, how, generic_rule=False):
    """Equal to the reference (exact family) or within the derived bound (generic family); entries all of whose terms are
    zero -- input slices no window reaches among them -- are exact zeros."""
    case = CF.ALL[name]
    ref, mag = CF.reference(name, rule, fam)
    got = got.detach().cpu()
    assert got.dtype == torch.float32 and got.shape == ref.shape, f"{how}: {got.dtype} {tuple(got.shape)} for {tuple(ref.shape)}"
    assert int(torch.count_nonzero(got[mag == 0])) == 0, f"{how}: non-zero entries where no term is"
    for d in case.expects["zero_depth"] if rule == "input" else ():
        assert int(torch.count_nonzero(got[:, :, :, d])) == 0, f"{how}: depth slice {d} is read by no window"
    if fam == "exact":
        bad = got.double() != ref
        assert not bool(bad.any()), f"{how}: {int(bad.sum())} of {bad.numel()} entries differ, first at {bad.nonzero()[0].tolist()}"
        return
    bound = CF.bound(case, rule, mag, generic_rule)
    err = (got.double() - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{name}/{rule} ({how}): worst error / bound = {ratio:.3g}")
    bad = err > bound
    assert not bool(bad.any()), f"{how}: {int(bad.sum())} entries beyond the bound, worst error / bound = {ratio:.3g}"


def forbidden(*a, **k):
    raise AssertionError("fell back to the torch rule")


@pytest.mark.parametrize("name,rule,fam", CF.RUNS)
def test_lowering_and_dispatch(name, rule, fam, monkeypatch):
    case = CF.ALL[name]
    module, x, M = CF.on_device(case, fam, DEV)
    served = rule == "weight" or case.expects["served"] == "hip"
    direct = CF.lower(case, rule, module, M, x)
    if served:
        assert direct is not None, f"{case.expects['lowering']} declined a case labelled as served"
        check(direct, name, rule, fam, "lowering")
        again = CF.lower(case, rule, module, M, x)
        assert torch.equal(direct, again), "two runs of the lowering differ"
        # the dispatch must reach the kernels: no vmap rule, no einsum, no autograd
        monkeypatch.setattr(ext, "_conv_weight_factor", forbidden)
        monkeypatch.setattr(torch, "einsum", forbidden)
        monkeypatch.setattr(torch.autograd, "grad", forbidden)
        through = CF.dispatch(case, rule, module, M, x)
        monkeypatch.undo()
        check(through, name, rule, fam, "dispatch")
        assert torch.equal(through, direct), "the dispatch and the lowering differ"
    else:
        assert direct is None, f"{case.expects['lowering']} serves a case labelled as declined ({case.expects['reason']})"
        through = CF.dispatch(case, rule, module, M, x)
        check(through, name, rule, fam, "dispatch, generic rule", generic_rule=True)
        if fam == "exact":   # (torch's own backward may add with atomics: only sums that are exact in any order repeat bit for bit)
            assert torch.equal(through, CF.dispatch(case, rule, module, M, x)), "two runs of the dispatch differ"


@pytest.fixture(scope="module")
def scalar_child(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("conv_family") / "conv_family.pt")
    env = dict(os.environ, VIVIT_CONV_MFMA="0")
    proc = subprocess.run([sys.executable, os.path.join(HERE, "conv_family_child.py"), out], stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, timeout=300, env=env)
    assert proc.returncode == 0, proc.stdout[-3000:]
    return torch.load(out)


@pytest.mark.parametrize("name,rule,fam", CF.MFMA_RUNS)
def test_matrix_pipe_cases_with_the_matrix_pipe_off(name, rule, fam, scalar_child):
    """VIVIT_CONV_MFMA=0.  Weight rule: the scalar kernel takes every slice, the same checks hold.  Input rule: the scalar
    kernel cannot hold these filter slices (tests/test_conv_family_refs_host.py asserts it of the mirror), so the lowering
    raises VIVIT_E_UNSUPPORTED -- which shows that the default run was on the matrix pipe -- and the dispatch falls through
    to the generic rule and still returns the reference."""
    res = scalar_child[(name, rule, fam)]
    if rule == "weight":
        check(res["direct"], name, rule, fam, "lowering, scalar kernel")
        check(res["dispatch"], name, rule, fam, "dispatch, scalar kernel")
        return
    assert res["direct"] == ("unsupported", _lib.VIVIT_E_UNSUPPORTED), f"the lowering returned {res['direct']!r}: the case is labelled mfma"
    check(res["dispatch"], name, rule, fam, "dispatch, generic rule", generic_rule=True)
