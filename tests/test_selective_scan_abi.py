"""csrc/selective_scan.hip: exports, prototypes and the refusals, all from host-side checks before any device call (no GPU; fake
pointers, as tests/test_depthwise_abi.py)."""
import os
import re

from vivit_amd import _lib

BADARG, WORKSPACE, UNSUPPORTED = -1, -2, -4
P = tuple(0x7F0000001000 + i * 0x10000000 for i in range(8))   # (fake device pointers)
NAMES = ("vivit_selective_scan_forward_f32", "vivit_selective_scan_rules_f32_workspace_bytes", "vivit_selective_scan_rules_f32")


def test_exported_with_the_headers_argument_counts():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vivit_hip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(_lib.SIGNATURES[name][1]) == args.count(",") + 1 and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.ABI_VERSION == 1008 and lib.vivit_hip_abi_version() == 1008   # exports were only added


def test_refusals_come_without_a_device():
    lib = _lib.load()
    fwd = lambda S=16, x=P[0]: lib.vivit_selective_scan_forward_f32(x, P[1], P[2], P[3], 2, 20, 70, S, 1, None)   # noqa: E731
    assert fwd(S=65) == UNSUPPORTED and fwd(x=None) == BADARG and fwd(S=0) == BADARG
    need = lib.vivit_selective_scan_rules_f32_workspace_bytes(3, 2, 20, 70, 16, 7)
    assert need > 0 and lib.vivit_selective_scan_rules_f32_workspace_bytes(3, 2, 20, 70, 65, 7) == 0
    rules = lambda S=16, M=P[0], want=7, ws=P[7], nb=need: lib.vivit_selective_scan_rules_f32(   # noqa: E731
        M, P[1], P[2], P[3], P[4], P[5], P[6], 3, 2, 20, 70, S, 1, want, ws, nb, None)
    assert rules(S=65) == UNSUPPORTED and rules(M=None) == BADARG and rules(want=0) == BADARG
    assert rules(nb=need - 1) == WORKSPACE and rules(ws=None) == WORKSPACE
    assert rules(S=65, nb=0) == UNSUPPORTED   # (before the workspace is looked at)
