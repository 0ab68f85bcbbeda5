"""Both Conv2d rule entry points (vivit_conv2d_weight_mjp_f32, vivit_conv2d_jac_t_f32) on every branch of their host planners,
against the fp64 CPU references of tests/conv_refs.py: the four row-tile instantiations of the weight rule's matrix-pipe
kernel, its tail step (OH OW % 4 != 0), its position splits with and without a tail and with idle waves, OW = 4, dilation,
asymmetric stride / padding / dilation, padding beyond the kernel extent, 1 x 1 kernels on a single row, and its three
reasons to fall back; the input rule's matrix-pipe kernel with one, several and ragged output-channel chunks, chunks together
with a split of the contraction, both row tiles, several trips, 1 x 1 kernels, strides beyond the kernel, the 1024 | 1025
boundary of the filter slice, and the scalar kernel's tiled and rows-per-workgroup bodies.  tests/test_conv_refs_host.py pins
every case to its branch.

Every case runs in this process (matrix pipe where the planner chooses it) and in a child with VIVIT_CONV_MFMA=0 (scalar
kernels), in two input families: exact (small integers: bit-equal to the fp64 reference) and generic (elementwise
(n + 2) eps sum|terms|).  Outputs are views between guard words, pre-filled with NaN (tests/conv_rules_child.py)."""
import os
import subprocess
import sys

import pytest
import torch

import conv_refs as R
import conv_rules_child as child
from vivit_amd._lib import VIVIT_E_UNSUPPORTED, VIVIT_OK

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WHERE = ["default", "child"]


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("conv_rules") / "conv_rules.pt")
    env = dict(os.environ, VIVIT_CONV_MFMA="0")
    proc = subprocess.run([sys.executable, os.path.join(HERE, "conv_rules_child.py"), out], stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, timeout=300, env=env)
    assert proc.returncode == 0, proc.stdout[-3000:]
    return {"default": child.run(), "child": torch.load(out)}


def check_result(res, rule, name, fam):
    """status OK, guards bit-unchanged, every element written, and the values: equal to the reference (exact family) or
    within the derived bound (generic family)."""
    assert res["status"] == VIVIT_OK, f"status {res['status']}"
    assert res["guards"], "a guard word around the output changed"
    got = res["out"]
    assert not bool(torch.isnan(got).any()), f"{int(torch.isnan(got).sum())} elements were never written"
    ref, bound = R.reference(rule, name, fam)
    ref, bound = ref.reshape(got.shape), bound.reshape(got.shape)
    if fam == "exact":
        bad = got.double() != ref
        assert torch.equal(got.double(), ref), f"{int(bad.sum())} of {bad.numel()} entries differ, first at {bad.nonzero()[0].tolist()}"
    else:
        err = (got.double() - ref).abs()
        bad = err > bound
        worst = (err / bound.clamp_min(1e-300))[bad].max().item() if bool(bad.any()) else 0.0
        print(f"{rule}/{name}: worst error / bound = {(err / bound.clamp_min(1e-300)).max().item():.3g}")
        assert not bool(bad.any()), f"{int(bad.sum())} entries beyond the bound, worst error / bound = {worst:.3g}"


@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name", [c.name for c in R.WEIGHT_CASES])
def test_weight_rule(name, where, fam, both):
    check_result(both[where][("weight", name, fam)], "weight", name, fam)


@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name", [c.name for c in R.INPUT_CASES])
def test_input_rule(name, where, fam, both):
    res = both[where][("input", name, fam)]
    if where == "child" and R.CASES["input"][name].expects["route"] == "mfma":
        # the one place where the route is observable: the scalar kernel cannot hold these filter slices, so with the matrix
        # pipe switched off the call is refused -- and must not have touched the output
        assert res["status"] == VIVIT_E_UNSUPPORTED, f"status {res['status']}: the case is labelled mfma"
        assert res["guards"] and bool(torch.isnan(res["out"]).all())
        return
    check_result(res, "input", name, fam)


def test_filter_slice_of_1024_runs_on_the_scalar_kernel(both):
    """Cout KH KW = 1024 is the last slice the scalar kernel takes: the child (matrix pipe off) serves it, 1025 it refuses."""
    for fam in R.FAMILIES:
        assert both["child"][("input", "1024-edge", fam)]["status"] == VIVIT_OK
        assert both["child"][("input", "1025-edge", fam)]["status"] == VIVIT_E_UNSUPPORTED
        assert both["default"][("input", "1025-edge", fam)]["status"] == VIVIT_OK


@pytest.mark.parametrize("name", R.TINY_FLOOR)
def test_tiny_wide_slices_run_on_the_matrix_pipe(name, both):
    """128 output channels x 3 x 3 on a 1 x 3 or 1 x 1 input (a Conv1d of length <= 3, the last stage of a net pooled to
    1 x 1): too wide for the scalar kernel, so the matrix pipe must take it however little work it is."""
    for fam in R.FAMILIES:
        res = both["default"][("input", name, fam)]
        assert res["status"] == VIVIT_OK, f"status {res['status']} (VIVIT_E_UNSUPPORTED = {VIVIT_E_UNSUPPORTED})"
        check_result(res, "input", name, fam)


@pytest.mark.parametrize("operand", ["M", "other", "out"])
@pytest.mark.parametrize("rule,name", [("weight", "rt2-Lmod2"), ("input", "wide-asym")])
def test_misaligned_operand(rule, name, operand):
    """Each operand in turn at an address that is 4 mod 16 (``other``: x of the weight rule, the weight of the input rule),
    on a matrix-pipe case: neither kernel may assume more than the alignment of a float."""
    assert R.CASES[rule][name].expects["route"] == "mfma"
    check_result(child.run_case(rule, name, "exact", misalign=operand), rule, name, "exact")
