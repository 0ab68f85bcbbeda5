"""``vivit_attention_bias_factor_f32`` and its workspace query (include/vivit_hip.h): the refusing half of the entry point.

No GPU is needed and none is used: every call below must be refused by the host-side checks before anything is enqueued (as
tests/test_attention_scoremod_abi.py does for the score-modifier entry point; the pointers are fake non-null addresses that the host
never dereferences).

On the commit before the feature every test of this file fails: the library exports neither symbol."""
import os
import re

import pytest

from vivit_amd import _lib

OK, BADARG, WORKSPACE, LAUNCH, UNSUPPORTED = 0, -1, -2, -3, -4
P = 0x7F0000001000  # fake device pointers
M, QKV, OUT, GB, WS, LEN, BIAS, IDX = (P, P + 0x10000000, P + 0x20000000, P + 0x30000000, P + 0x60000000, P + 0x70000000, P + 0x78000000,
                                       P + 0x7C000000)
BIG = 1 << 40
NAMES = ("vivit_attention_bias_factor_f32_workspace_bytes", "vivit_attention_bias_factor_f32")
INF, NAN = float("inf"), float("nan")
SHAPES = [(1, 1, 1, 1, 1, 1), (3, 2, 17, 4, 2, 20), (1, 1, 32, 2, 1, 16), (2, 3, 33, 2, 2, 17), (10, 64, 197, 6, 2, 64), (3, 2, 4097, 8, 1, 128),
          (10, 4, 512, 32, 8, 128), (3, 2, 17, 4, 4, 20), (5, 1, 64, 3, 3, 33), (9, 4, 161, 6, 3, 128), (262140, 1, 1, 1, 1, 16)]
REFUSED = [(3, 2, 17, 4, 2, 129), (3, 2, 17, 4, 3, 20), (0, 2, 17, 4, 2, 20), (3, 2, 0, 4, 2, 20), (3, 2, 17, 4, 0, 20), (1 << 20, 2, 17, 4, 2, 20),
           (3, 2, (1 << 31) - 16, 4, 2, 20), (3, 2, 17, -4, 2, 20), (131071, 1, 5, 1, 1, 33)]


def call(V=3, N=2, T=17, H=4, Hkv=2, d=20, M=M, qkv=QKV, out=OUT, Gb=GB, ws=WS, wsb=BIG, causal=0, lengths=LEN, window=5, softcap=0.0,
         bias=BIAS, index=IDX, R=33):
    return _lib.load().vivit_attention_bias_factor_f32(M, qkv, out, Gb, V, N, T, H, Hkv, d, 0.25, causal, lengths, window, softcap, bias, index,
                                                       R, ws, wsb, None)


def need(V=3, N=2, T=17, H=4, Hkv=2, d=20):
    return _lib.load().vivit_attention_bias_factor_f32_workspace_bytes(V, N, T, H, Hkv, d)


def scoremod(*shape):
    return _lib.load().vivit_attention_scoremod_jac_t_f32_workspace_bytes(*shape)


def test_symbols_are_exported_bound_and_declared():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "vivit_hip.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert re.search(r"\b(size_t|int) " + name + r"\(", header), name
    assert re.search(r"float softcap, const float \*bias, const int32_t \*index, int64_t R,\s+void \*workspace", header)
    assert len(_lib.SIGNATURES[NAMES[1]][1]) == 21 and len(_lib.SIGNATURES[NAMES[0]][1]) == 6
    assert _lib.ABI_VERSION == 1008 and lib.vivit_hip_abi_version() == 1008   # exports were only added


@pytest.mark.parametrize("shape", SHAPES)
def test_workspace_exceeds_the_scoremod_entrys_by_the_partial_sums_at_most(shape):
    V, N, T, H, Hkv, d = shape
    base, mine = scoremod(*shape), need(*shape)
    assert 0 < base < mine <= base + 4 * 64 * (2 * ((T + 31) // 32) - 1) * V * N * H


@pytest.mark.parametrize("shape", SHAPES + REFUSED)
def test_query_and_refusals_are_where_the_scoremod_entrys_are(shape):
    V, N, T, H, Hkv, d = shape
    assert (need(*shape) == 0) == (scoremod(*shape) == 0)
    kw = dict(V=V, N=N, T=T, H=H, Hkv=Hkv, d=d)
    lib = _lib.load()
    theirs = lib.vivit_attention_scoremod_jac_t_f32(M, QKV, OUT, GB, V, N, T, H, Hkv, d, 0.25, 0, LEN, 5, 0.0, BIAS, None, 0, None)
    assert call(ws=None, wsb=0, **kw) == theirs
    assert theirs == (WORKSPACE if need(*shape) else theirs) and theirs in (BADARG, UNSUPPORTED, WORKSPACE)


@pytest.mark.parametrize("softcap", [-1.0, -0.0001, -INF, INF, NAN])
def test_a_cap_that_is_negative_or_not_finite_is_refused(softcap):
    assert call(softcap=softcap) == BADARG
    assert call(softcap=softcap, ws=None, wsb=0) == BADARG     # (before the workspace is looked at)
    assert call(softcap=softcap, d=129) == BADARG              # (and before the shape is)


@pytest.mark.parametrize("which", ["M", "qkv", "out", "Gb", "bias", "index"])
def test_null_operands_are_refused(which):
    assert call(**{which: None}) == BADARG
    assert call(**{which: None}, lengths=None, window=0, softcap=2.0) == BADARG
    assert call(**{which: None}, ws=None, wsb=0) == BADARG
    assert call(**{which: None}, d=129) == BADARG


@pytest.mark.parametrize("R", [0, -1, -(1 << 40)])
def test_a_table_without_columns_is_refused(R):
    assert call(R=R) == BADARG and call(R=R, ws=None, wsb=0) == BADARG and call(R=R, d=129) == BADARG


@pytest.mark.parametrize("which", ["V", "N", "T", "H", "Hkv", "d"])
def test_non_positive_sizes_are_refused(which):
    assert call(**{which: 0}) == BADARG and call(**{which: -1}) == BADARG
    assert need(**{which: 0}) == 0 and need(**{which: -1}) == 0


def test_a_negative_window_and_unequal_groups_are_refused():
    assert call(window=-1) == BADARG and call(window=-1, ws=None, wsb=0) == BADARG
    assert call(H=4, Hkv=3) == BADARG


def test_unsupported_shapes_are_refused_before_the_workspace_check():
    assert call(d=129) == UNSUPPORTED and call(d=129, ws=None, wsb=0) == UNSUPPORTED
    assert call(d=128, wsb=16) == WORKSPACE   # (d = 128 itself is supported)
    assert call(V=1 << 20, ws=None, wsb=0) == UNSUPPORTED
    assert call(T=(1 << 31) - 16, ws=None, wsb=0) == UNSUPPORTED


@pytest.mark.parametrize("shape", [(3, 2, 17, 4, 2, 20), (1, 1, 1, 2, 1, 1), (10, 64, 197, 6, 3, 64), (3, 2, 65, 3, 1, 128)])
def test_short_workspace_is_refused(shape):
    want = need(*shape)
    V, N, T, H, Hkv, d = shape
    kw = dict(V=V, N=N, T=T, H=H, Hkv=Hkv, d=d)
    assert want > 0
    assert call(wsb=want - 1, **kw) == WORKSPACE
    assert call(wsb=scoremod(*shape), **kw) == WORKSPACE       # (the input rule's workspace is too short)
    assert call(ws=None, wsb=want, **kw) == WORKSPACE and call(ws=None, wsb=0, **kw) == WORKSPACE


def test_every_accepted_argument_reaches_the_workspace_check():
    for softcap in (0.0, 1e-30, 0.5, 50.0, 3e38):
        for bias, index in ((BIAS, IDX), (BIAS + 4, IDX + 4)):   # (neither needs an alignment beyond four bytes)
            for lengths, window, causal, R in ((None, 0, 0, 1), (LEN, 0, 1, 33), (None, 1, 1, 8), (LEN, 1 << 62, 0, 1 << 40)):
                kw = dict(softcap=softcap, bias=bias, index=index, lengths=lengths, window=window, causal=causal, R=R)
                assert call(wsb=16, **kw) == WORKSPACE and call(ws=None, wsb=0, **kw) == WORKSPACE
