"""Workspace queries of the GEMM planner (csrc/gemm_plan.h: plan_<route>) against a recorded table.  Host only, no device.

tests/golden/gemm_workspace.json holds what vivit_gemm_f32_workspace_bytes(m, n, k) and vivit_gram_syrk_f32_workspace_bytes(n, p)
answered BEFORE the per-route planners replaced the separately written query, at shapes on both sides of every route boundary
(tests/golden/make_golden.py: _gemm_workspace_shapes), in the default environment.  The answers must stay EQUAL, not merely
sufficient: callers size and carve one buffer from them, and a query that drifts from its launch is how a route ends up
refused (or, worse, over-running) on shapes nobody tried.
"""
import json
import os

import pytest

from vivit_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
SWITCHES = ("VIVIT_GEMM256", "VIVIT_GEMM_SPLIT", "VIVIT_GEMM_BXSPLITK", "VIVIT_GEMM64", "VIVIT_GEMM64_BX", "VIVIT_GEMM_TSK", "VIVIT_BX_ASM")


@pytest.fixture(scope="module")
def table():
    assert not [s for s in SWITCHES if s in os.environ], "the table was recorded in the default environment"
    with open(os.path.join(HERE, "golden", "gemm_workspace.json")) as f:
        return json.load(f)


def test_table_covers_the_route_boundaries(table):
    gemm = {tuple(r[:3]) for r in table["gemm"]}
    syrk = {tuple(r[:2]) for r in table["syrk"]}
    assert len(gemm) == len(table["gemm"]) and len(syrk) == len(table["syrk"])
    for shape in [(2560, 5120, 511), (2560, 5120, 512), (2816, 4608, 4096),             # 256 tile: K 511 | 512, 200 | 198 tiles
                  (2560, 2560, 16368), (2560, 2560, 16384), (1536, 4352, 16384),        # split-K: K, 100 | 102 tiles
                  (64, 2048, 2048), (65, 2048, 2048), (64, 2047, 2048), (64, 2304, 4100),   # 64-row route
                  (48, 1024, 2048), (48, 1025, 2048), (48, 700, 2047), (48, 700, 8190),     # deep-K small-output route
                  (300, 300, 1008), (300, 300, 1009),                                       # 128 tile: 63 | 64 K tiles
                  (4096, 4096, 2071), (1000, 1300, 20480), (64, 2304, 4096), (1, 2048, 2048), (48, 700, 8192), (8, 5000, 3000),
                  (300, 300, 5001)]:
        assert shape in gemm, shape
    for shape in [(40960, 401408), (4864, 4096), (5120, 4096), (3328, 16384), (3584, 16384), (512, 2048)]:
        assert shape in syrk, shape


def test_gemm_workspace_queries_are_unchanged(table):
    L = _lib.load()
    got = [[m, n, k, L.vivit_gemm_f32_workspace_bytes(m, n, k)] for m, n, k, _ in table["gemm"]]
    assert got == table["gemm"]


def test_syrk_workspace_queries_are_unchanged(table):
    L = _lib.load()
    got = [[n, p, L.vivit_gram_syrk_f32_workspace_bytes(n, p)] for n, p, _ in table["syrk"]]
    assert got == table["syrk"]
