"""``vivit_attention_forward_f32`` and ``vivit_attention_cross_forward_f32`` (include/vivit_hip.h): the refusing half of the two entry
points.  No GPU is needed and none is used: every call is refused by the host-side checks before anything is enqueued (the pointers
are fake non-null addresses that the host never dereferences, as in tests/test_attention_wide_abi.py)."""
import os
import re

import pytest

from vivit_amd import _lib

BADARG, UNSUPPORTED = -1, -4
P = 0x7F0000001000  # fake device pointers
QKV, KV, OUT, LSE, LEN, BIAS = P, P + 0x10000000, P + 0x20000000, P + 0x30000000, P + 0x70000000, P + 0x78000000
NAMES = ("vivit_attention_forward_f32", "vivit_attention_cross_forward_f32")


def call(N=2, T=17, H=4, Hkv=2, d=64, qkv=QKV, out=OUT, lse=LSE, causal=1, lengths=LEN, window=5, softcap=1.5, bias=BIAS):
    return _lib.load().vivit_attention_forward_f32(qkv, out, lse, N, T, H, Hkv, d, 0.25, causal, lengths, window, softcap, bias, None)


def cross(N=2, Tq=17, Tk=40, H=4, Hkv=2, d=64, q=QKV, kv=KV, out=OUT, lse=LSE):
    return _lib.load().vivit_attention_cross_forward_f32(q, kv, out, lse, N, Tq, Tk, H, Hkv, d, 0.25, LEN, None, None)


def test_symbols_are_exported_bound_and_declared():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "vivit_hip.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\bint " + name + r"\(", header), name


@pytest.mark.parametrize("softcap,bias", [(1.5, BIAS), (0.0, None)])
def test_self_attention_refusals_follow_the_order_of_the_scoremod_entry(softcap, bias):
    kw = dict(softcap=softcap, bias=bias)
    for d in (129, 192, 256, 512):   # the torch formula's head dimensions
        assert call(d=d, **kw) == UNSUPPORTED
    for bad in (-1.0, float("inf"), float("nan")):   # the cap first: before the operands and the shape
        assert call(softcap=bad, bias=bias, qkv=None, d=129) == BADARG
    for which in ("qkv", "out"):
        assert call(**{which: None}, d=129, **kw) == BADARG
    assert call(window=-1, d=129, **kw) == BADARG
    for which in ("N", "T", "H", "Hkv", "d"):
        assert call(**{which: 0}, **kw) == BADARG and call(**{which: -1}, **kw) == BADARG
    assert call(H=4, Hkv=3, **kw) == BADARG
    assert call(T=(1 << 31) - 16, **kw) == UNSUPPORTED and call(N=1 << 31, lse=None, **kw) == UNSUPPORTED


def test_cross_attention_refusals_follow_the_order_of_the_rule_entry():
    for d in (129, 256):
        assert cross(d=d) == UNSUPPORTED
    for which in ("q", "kv", "out"):
        assert cross(**{which: None}, d=129) == BADARG
    for which in ("N", "Tq", "Tk", "H", "Hkv", "d"):
        assert cross(**{which: 0}) == BADARG and cross(**{which: -1}) == BADARG
    assert cross(H=4, Hkv=3) == BADARG
    assert cross(Tq=(1 << 31) - 16) == UNSUPPORTED and cross(Tk=(1 << 31) - 16, lse=None) == UNSUPPORTED
