"""Child process of tests/test_conv_family_gpu.py: the ``mfma``-labelled cases of tests/conv_family_refs.py through their
lowering and through the dispatch, with the environment the parent set (VIVIT_CONV_MFMA=0 is read once per process, so
the scalar kernels serve or refuse every slice); results as a .pt file.

Per (case, rule, family): ``{"direct": tensor | ("unsupported", status), "dispatch": tensor}``.

usage: python conv_family_child.py OUT.pt
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import conv_family_refs as CF  # noqa: E402
from vivit_amd import _lib  # noqa: E402

DEV = torch.device("cuda:0")


def run_one(name, rule, fam):
    case = CF.ALL[name]
    module, x, M = CF.on_device(case, fam, DEV)
    try:
        direct = CF.lower(case, rule, module, M, x).cpu()
    except _lib.VivitHipError as exc:
        direct = ("unsupported" if exc.status == _lib.VIVIT_E_UNSUPPORTED else "error", exc.status)
    return {"direct": direct, "dispatch": CF.dispatch(case, rule, module, M, x).cpu()}


def run():
    torch.cuda.set_device(DEV)
    return {key: run_one(*key) for key in CF.MFMA_RUNS}


if __name__ == "__main__":
    torch.save(run(), sys.argv[1])
