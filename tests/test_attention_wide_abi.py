"""``vivit_attention_wide_jac_t_f32`` and its workspace query (include/vivit_hip.h): the refusing half of the entry point and the
workspace size.  No GPU is needed and none is used: every call is refused by the host-side checks before anything is enqueued (the
pointers are fake non-null addresses that the host never dereferences, as in tests/test_attention_scoremod_abi.py)."""
import os
import re

import pytest

from vivit_amd import _lib

OK, BADARG, WORKSPACE, LAUNCH, UNSUPPORTED = 0, -1, -2, -3, -4
P = 0x7F0000001000  # fake device pointers
M, QKV, OUT, G, WS, LEN, BIAS = P, P + 0x10000000, P + 0x20000000, P + 0x30000000, P + 0x60000000, P + 0x70000000, P + 0x78000000
BIG = 1 << 40
NAMES = ("vivit_attention_wide_jac_t_f32_workspace_bytes", "vivit_attention_wide_jac_t_f32")
MODS = [(1.5, BIAS), (0.0, None)]   # the score-modifier instances and the plain ones


def call(V=3, N=2, T=17, H=4, Hkv=2, d=192, M=M, qkv=QKV, out=OUT, G=G, ws=WS, wsb=BIG, causal=1, lengths=LEN, window=5, softcap=1.5,
         bias=BIAS):
    return _lib.load().vivit_attention_wide_jac_t_f32(M, qkv, out, G, V, N, T, H, Hkv, d, 0.25, causal, lengths, window, softcap, bias, ws,
                                                      wsb, None)


def need(V=3, N=2, T=17, H=4, Hkv=2, d=192):
    return _lib.load().vivit_attention_wide_jac_t_f32_workspace_bytes(V, N, T, H, Hkv, d)


def test_symbols_are_exported_bound_and_declared():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "vivit_hip.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\b(size_t|int) " + name + r"\(", header), name
    assert _lib.SIGNATURES[NAMES[1]] == _lib.SIGNATURES["vivit_attention_scoremod_jac_t_f32"]
    assert _lib.SIGNATURES[NAMES[0]] == _lib.SIGNATURES["vivit_attention_scoremod_jac_t_f32_workspace_bytes"]


@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 1, 129), (3, 2, 17, 4, 2, 192), (10, 4, 512, 16, 8, 256), (5, 3, 4097, 8, 1, 255)])
def test_workspace_is_lse_and_the_row_dots(shape):
    V, N, T, H, Hkv, d = shape
    assert need(*shape) == (N * H * T * 4 + 255) // 256 * 256 + V * N * H * T * 4


@pytest.mark.parametrize("softcap,bias", MODS)
def test_refusals_follow_the_order_of_the_scoremod_entry(softcap, bias):
    kw = dict(softcap=softcap, bias=bias)
    for d in (1, 64, 128, 257, 512):   # the narrow entries' head dimensions, and those beyond every kernel
        assert call(d=d, **kw) == UNSUPPORTED and call(d=d, ws=None, wsb=0, **kw) == UNSUPPORTED and need(d=d) == 0
    for d in (129, 256):
        assert call(d=d, wsb=16, **kw) == WORKSPACE and call(d=d, ws=None, **kw) == WORKSPACE and need(d=d) > 0
        assert call(d=d, wsb=need(d=d) - 1, **kw) == WORKSPACE
    for bad in (-1.0, float("inf"), float("nan")):   # the cap first: before the operands, the shape and the workspace
        assert call(softcap=bad, bias=bias, M=None, d=64, ws=None, wsb=0) == BADARG
    for which in ("M", "qkv", "out", "G"):
        assert call(**{which: None}, d=64, **kw) == BADARG
    assert call(window=-1, d=64, ws=None, wsb=0, **kw) == BADARG
    for which in ("V", "N", "T", "H", "Hkv", "d"):
        assert call(**{which: 0}, **kw) == BADARG and call(**{which: -1}, **kw) == BADARG and need(**{which: 0}) == 0
    assert call(H=4, Hkv=3, **kw) == BADARG and need(H=4, Hkv=3) == 0
    assert call(V=1 << 20, ws=None, wsb=0, **kw) == UNSUPPORTED and call(T=(1 << 31) - 16, ws=None, wsb=0, **kw) == UNSUPPORTED
