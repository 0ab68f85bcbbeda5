"""Child process of tests/test_conv_rules_gpu.py: every case of tests/conv_refs.py through the C ABI of the two Conv2d rule
entry points, with the environment the parent set (VIVIT_CONV_MFMA is read once per process); results as a .pt file.  The
parent imports this module as well and calls :func:`run` in-process for the default route.

The entry points are called through ``_lib.load()`` directly, not through the ``kernels.*`` wrappers: those allocate the
result with ``torch.empty`` and would hide an element nobody wrote or a write past the end.  Here every output is a view
into a buffer pre-filled with NaN that has GUARD floats of SENTINEL in front of it and GUARD behind it.

usage: python conv_rules_child.py OUT.pt
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import conv_refs as R  # noqa: E402
from epilogue_refs import SENTINEL  # noqa: E402
from vivit_amd import _lib  # noqa: E402

DEV = torch.device("cuda:0")
GUARD = 64


def guarded(numel, shift=0):
    """(buffer, view of ``numel`` floats): the view is NaN, everything around it SENTINEL; ``shift = 1`` makes the view's
    address 4 mod 16."""
    buf = torch.full((GUARD + shift + numel + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[GUARD + shift:GUARD + shift + numel]
    view.fill_(float("nan"))
    assert view.data_ptr() % 16 == 4 * shift
    return buf, view


def guards_intact(buf, numel, shift=0):
    want = torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32).item()
    bits = buf.view(torch.int32)
    return bool((bits[:GUARD + shift] == want).all()) and bool((bits[GUARD + shift + numel:] == want).all())


def call(rule, g, M, other, out, rows=None):
    """The ABI call of a rule on device operands; returns the status."""
    OH, OW = R.out_hw(*g[2:])
    rows = R.V_SLICES * R.N_BATCH if rows is None else rows
    lib = _lib.load()
    stream = torch.cuda.current_stream(DEV).cuda_stream
    geo = (g.Cout, g.k[0], g.k[1], OH, OW, g.s[0], g.s[1], g.p[0], g.p[1], g.d[0], g.d[1])
    if rule == "weight":
        return lib.vivit_conv2d_weight_mjp_f32(M.data_ptr(), other.data_ptr(), out.data_ptr(), rows, R.N_BATCH, g.Cin, g.H, g.W, *geo, stream)
    return lib.vivit_conv2d_jac_t_f32(M.data_ptr(), other.data_ptr(), out.data_ptr(), rows, g.Cin, g.H, g.W, *geo, stream)


def out_shape(rule, g):
    if rule == "weight":
        return (R.V_SLICES, R.N_BATCH, g.Cout, g.Cin * g.k[0] * g.k[1])
    return (R.V_SLICES, R.N_BATCH, g.Cin, g.H, g.W)


def run_case(rule, name, fam, misalign=None):
    """One case: {"status", "out" (CPU tensor; NaN where nothing was written), "guards" (bit-unchanged)}.  ``misalign``:
    "M", "other" or "out" -- that operand at an address that is 4 mod 16."""
    g = R.CASES[rule][name].geom
    M, other = (t.to(DEV) for t in R.make_case(rule, name, fam))
    if misalign == "M":
        M = R.misaligned(M)
    if misalign == "other":
        other = R.misaligned(other)
    shape = out_shape(rule, g)
    numel, shift = int(torch.Size(shape).numel()), int(misalign == "out")
    buf, view = guarded(numel, shift)
    status = call(rule, g, M, other, view)
    torch.cuda.synchronize(DEV)
    return {"status": int(status), "out": view.cpu().reshape(shape), "guards": guards_intact(buf, numel, shift)}


def run():
    torch.cuda.set_device(DEV)
    return {(rule, c.name, fam): run_case(rule, c.name, fam) for rule, cases in (("weight", R.WEIGHT_CASES), ("input", R.INPUT_CASES))
            for c in cases for fam in R.FAMILIES}


if __name__ == "__main__":
    torch.save(run(), sys.argv[1])
