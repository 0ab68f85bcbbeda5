"""csrc/ssd.hip: exports, prototypes and the refusals, all from host-side checks before any device call (no GPU; fake pointers, as
tests/test_selective_scan_abi.py)."""
import os
import re

from vivit_amd import _lib

BADARG, WORKSPACE, UNSUPPORTED = -1, -2, -4
F = tuple(0x7F0000001000 + i * 0x10000000 for i in range(10))   # (fake device pointers)
NAMES = ("vivit_ssd_forward_f32", "vivit_ssd_rules_f32_workspace_bytes", "vivit_ssd_rules_f32")


def test_exported_with_the_headers_argument_counts():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vivit_hip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(_lib.SIGNATURES[name][1]) == args.count(",") + 1 and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.ABI_VERSION == 1008 and lib.vivit_hip_abi_version() == 1008   # exports were only added


def test_refusals_come_without_a_device():
    lib = _lib.load()
    fwd = lambda P=16, S=16, G=1, x=F[0]: lib.vivit_ssd_forward_f32(x, F[1], F[2], F[3], F[4], 2, 70, 3, P, S, G, 1, None)   # noqa: E731
    assert fwd(S=129) == UNSUPPORTED and fwd(P=65) == UNSUPPORTED and fwd(x=None) == BADARG and fwd(S=0) == BADARG and fwd(G=2) == BADARG
    need = lib.vivit_ssd_rules_f32_workspace_bytes(3, 2, 70, 3, 16, 16, 1, 15)
    assert need > 0 and lib.vivit_ssd_rules_f32_workspace_bytes(3, 2, 70, 3, 16, 16, 1, 4) == 0
    assert lib.vivit_ssd_rules_f32_workspace_bytes(3, 2, 70, 3, 16, 129, 1, 15) == 0
    assert lib.vivit_ssd_rules_f32_workspace_bytes(3, 2, 70, 3, 65, 16, 1, 15) == 0
    rules = lambda P=16, S=16, M=F[0], want=15, ws=F[9], nb=need: lib.vivit_ssd_rules_f32(   # noqa: E731
        M, F[1], F[2], F[3], F[4], F[5], F[6], F[7], F[8], 3, 2, 70, 3, P, S, 1, 1, want, ws, nb, None)
    assert rules(S=129) == UNSUPPORTED and rules(P=65) == UNSUPPORTED and rules(M=None) == BADARG and rules(want=0) == BADARG
    assert rules(want=16) == BADARG and rules(nb=need - 1) == WORKSPACE and rules(ws=None) == WORKSPACE
    assert rules(S=129, nb=0) == UNSUPPORTED   # (before the workspace is looked at)
