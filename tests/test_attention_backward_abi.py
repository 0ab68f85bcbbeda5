"""``vivit_attention_backward_f32`` and ``vivit_attention_cross_backward_f32`` (include/vivit_hip.h) with their workspace queries: the
refusing half.  No GPU is needed and none is used: every call is refused by the host-side checks before anything is enqueued (the
pointers are fake non-null addresses that the host never dereferences, as in tests/test_attention_forward_abi.py).

On the commit before the feature this whole file fails: the symbols do not exist."""
import os
import re

import pytest

from vivit_amd import _lib

BADARG, UNSUPPORTED, WORKSPACE = -1, -4, -2
P = 0x7F0000001000  # fake device pointers
DOUT, QKV, KV, OUT, LSE, DQ, DKV, LEN, BIAS, WS = (P + k * 0x10000000 for k in range(10))
NAMES = ("vivit_attention_backward_f32", "vivit_attention_cross_backward_f32")


def self_bytes(N=2, T=17, H=4, Hkv=2, d=64):
    return _lib.load().vivit_attention_backward_f32_workspace_bytes(N, T, H, Hkv, d)


def cross_bytes(N=2, Tq=17, Tk=40, H=4, Hkv=2, d=64):
    return _lib.load().vivit_attention_cross_backward_f32_workspace_bytes(N, Tq, Tk, H, Hkv, d)


def call(N=2, T=17, H=4, Hkv=2, d=64, dout=DOUT, qkv=QKV, out=OUT, lse=LSE, dqkv=DQ, window=5, softcap=1.5, bias=BIAS, ws=WS, ws_bytes=None):
    ws_bytes = self_bytes(N, T, H, Hkv, d) if ws_bytes is None else ws_bytes
    return _lib.load().vivit_attention_backward_f32(dout, qkv, out, lse, dqkv, N, T, H, Hkv, d, 0.25, 1, LEN, window, softcap, bias, ws,
                                                    ws_bytes, None)


def cross(N=2, Tq=17, Tk=40, H=4, Hkv=2, d=64, dout=DOUT, q=QKV, kv=KV, out=OUT, lse=LSE, dq=DQ, dkv=DKV, ws=WS, ws_bytes=None):
    ws_bytes = cross_bytes(N, Tq, Tk, H, Hkv, d) if ws_bytes is None else ws_bytes
    return _lib.load().vivit_attention_cross_backward_f32(dout, q, kv, out, lse, dq, dkv, N, Tq, Tk, H, Hkv, d, 0.25, LEN, None, ws,
                                                          ws_bytes, None)


def test_symbols_are_exported_bound_and_declared():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "vivit_hip.h")).read()
    for name in NAMES:
        for symbol, kind in ((name, "int"), (name + "_workspace_bytes", "size_t")):
            assert symbol in _lib.SIGNATURES and hasattr(lib, symbol)
            assert re.search(r"\b" + kind + " " + symbol + r"\(", header), symbol
    assert lib.vivit_hip_abi_version() == 1008   # exports were only added


def test_the_workspace_is_d_alone_and_zero_for_refused_arguments():
    assert self_bytes() == 2 * 4 * 17 * 4 and cross_bytes() == 2 * 4 * 17 * 4   # D [N, H, Tq] floats, whatever Tk
    for kw in (dict(d=129), dict(d=256), dict(N=0), dict(H=4, Hkv=3), dict(d=-1)):
        assert self_bytes(**kw) == 0 and cross_bytes(**kw) == 0, kw
    assert self_bytes(T=(1 << 31) - 16) == 0 and cross_bytes(Tk=0) == 0 and cross_bytes(Tk=(1 << 31) - 16) == 0


@pytest.mark.parametrize("softcap,bias", [(1.5, BIAS), (0.0, None)])
def test_self_attention_refusals_follow_the_order_of_the_forward_entry(softcap, bias):
    kw = dict(softcap=softcap, bias=bias)
    for d in (129, 256):   # before the workspace is looked at
        assert call(d=d, ws=None, ws_bytes=0, **kw) == UNSUPPORTED
    for bad in (-1.0, float("inf"), float("nan")):   # the cap first: before the operands and the shape
        assert call(softcap=bad, bias=bias, qkv=None, d=129) == BADARG
    for which in ("dout", "qkv", "out", "lse", "dqkv"):
        assert call(**{which: None}, d=129, **kw) == BADARG
    assert call(window=-1, d=129, **kw) == BADARG
    for which in ("N", "T", "H", "Hkv", "d"):
        assert call(**{which: 0}, **kw) == BADARG and call(**{which: -1}, **kw) == BADARG
    assert call(H=4, Hkv=3, **kw) == BADARG
    assert call(T=(1 << 31) - 16, **kw) == UNSUPPORTED and call(N=1 << 31, **kw) == UNSUPPORTED
    assert call(ws=None, **kw) == WORKSPACE and call(ws_bytes=self_bytes() - 1, **kw) == WORKSPACE


def test_cross_attention_refusals_follow_the_order_of_the_forward_entry():
    for d in (129, 256):
        assert cross(d=d, ws=None, ws_bytes=0) == UNSUPPORTED
    for which in ("dout", "q", "kv", "out", "lse"):
        assert cross(**{which: None}, d=129) == BADARG
    assert cross(dq=None, dkv=None, d=129) == BADARG
    for which in ("N", "Tq", "Tk", "H", "Hkv", "d"):
        assert cross(**{which: 0}) == BADARG and cross(**{which: -1}) == BADARG
    assert cross(H=4, Hkv=3) == BADARG
    assert cross(Tq=(1 << 31) - 16) == UNSUPPORTED and cross(Tk=(1 << 31) - 16) == UNSUPPORTED
    for side in (dict(), dict(dq=None), dict(dkv=None)):   # either result alone is a call like the full one
        assert cross(ws=None, **side) == WORKSPACE and cross(ws_bytes=cross_bytes() - 1, **side) == WORKSPACE
