"""Workspace queries of the eigensolver entries against a recorded table.  Host only, no device.

tests/golden/eig_workspace.json holds what every public eigensolver query (vivit_symeig_f32, _symeigvals_batched_f32,
_symeig_reduce_f32, _symeig_select_f32, _symeig_select_batched_f32, _sytrd_f32, _stedc_f32, _sy2sb_f32, _sy2sb_panel_qr_f32,
_sb2st_f32, _q2_apply_f32, each with _workspace_bytes appended) answered BEFORE every workspace got one layout function that
both sizes and carves it (csrc/eig_internal.h: Arena), at sizes on both sides of every boundary the layouts branch on
(tests/golden/make_golden.py: _eig_workspace_rows).  The answers must stay EQUAL: callers allocate exactly what a query
says, and the regions inside keep their offsets only while the sizes in front of them do.

What the answers depend on besides the shape: the route switches VIVIT_TWO_STAGE and VIVIT_SYTRD_PERSIST (use_two_stage,
sytrd_persist_ok), VIVIT_Q2_SLIDE / VIVIT_Q2_SLIDE_MIN_ROWS (q2_slide_possible) and the VIVIT_GEMM* switches of the GEMM
planner (gemm_workspace_bytes) -- all environment -- and the device through ONE call: device_cu_count() in sytrd_persist_ok,
which use_two_stage asks for n <= 2048.  With VIVIT_SYTRD_PERSIST=0 that call is never reached, so the table holds on a box
with or without a GPU.  The switches are read once per process: each of the three environments (VIVIT_TWO_STAGE unset, 0, 1)
is asked in a child process.
"""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

CHILD = """
import json, sys
from vivit_amd import _lib
L = _lib.load()
rows = json.load(open(sys.argv[1]))[sys.argv[2]]
print(json.dumps([r[:-1] + [getattr(L, r[0] + "_workspace_bytes")(*r[1:-1])] for r in rows]))
"""


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(HERE, "golden", "eig_workspace.json")) as f:
        return json.load(f)


def test_table_covers_the_layout_boundaries(table):
    assert sorted(table) == ["0", "1", "unset"]
    for rows in table.values():
        have = {tuple(r[:-1]) for r in rows}
        assert len(have) == len(rows)
        sizes = (128, 129,                                 # two-stage guard n > 2 TS_NB (reached with VIVIT_TWO_STAGE=1)
                 192, 193,                                 # single workgroup | multi-kernel solver
                 1280, 1281,                               # one-XCD batched limit
                 2047, 2048, 2049,                         # use_two_stage crossover
                 4095, 4096, 8191, 8192, 16383, 16384,     # bt_nsub steps
                 4097, 4100,                               # n % 4 != 0: no sliding-window Q2
                 40960)                                    # bench size
        for n in sizes:
            for q in (("vivit_symeig_f32", n, 0), ("vivit_symeig_f32", n, 1), ("vivit_symeig_reduce_f32", n), ("vivit_sytrd_f32", n),
                      ("vivit_stedc_f32", n, 0), ("vivit_stedc_f32", n, 1), ("vivit_sy2sb_f32", n), ("vivit_sy2sb_panel_qr_f32", n),
                      ("vivit_sb2st_f32", n), ("vivit_q2_apply_f32", n)):
                assert q in have, q
            for K in (1, 256, 257, n):                     # SELECT_STEIN_MAX = 256
                assert ("vivit_symeig_select_f32", n, K) in have
                for batch in (1, 7, 8, 9):                 # PERSIST_MAX_BATCH = 8
                    assert ("vivit_symeigvals_batched_f32", n, batch) in have
                    assert ("vivit_symeig_select_batched_f32", n, batch, K) in have
    # the environments differ where they should: the forced two-stage layouts are other layouts
    answers = {k: {tuple(r[:-1]): r[-1] for r in v} for k, v in table.items()}
    assert answers["1"]["vivit_symeig_reduce_f32", 300] != answers["0"]["vivit_symeig_reduce_f32", 300]
    assert answers["unset"]["vivit_symeig_reduce_f32", 4096] == answers["1"]["vivit_symeig_reduce_f32", 4096]
    assert answers["unset"]["vivit_symeig_reduce_f32", 2047] == answers["0"]["vivit_symeig_reduce_f32", 2047]


@pytest.mark.parametrize("key", ["unset", "0", "1"])
def test_eig_workspace_queries_are_unchanged(table, key):
    from make_golden import EIG_WORKSPACE_ENVS, eig_workspace_env

    out = subprocess.run([sys.executable, "-c", CHILD, os.path.join(HERE, "golden", "eig_workspace.json"), key],
                         env=eig_workspace_env(EIG_WORKSPACE_ENVS[key]), cwd=os.path.dirname(HERE), stdout=subprocess.PIPE,
                         check=True, text=True).stdout
    got = json.loads(out.strip().splitlines()[-1])
    bad = [(g, w[-1]) for g, w in zip(got, table[key]) if g != w]
    assert not bad, bad[:20]
