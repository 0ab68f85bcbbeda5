"""``vivit_attention_scoremod_jac_t_f32`` and its workspace query (include/vivit_hip.h), and the activation kind 10 of
``vivit_act_jac_t_f32``: the refusing half of the entry points.

No GPU is needed and none is used: every call below must be refused by the host-side checks before anything is enqueued (as
tests/test_attention_masked_abi.py does for the masked entry point; the pointers are fake non-null addresses that the host never
dereferences)."""
import os
import re

import pytest

from vivit_amd import _lib

OK, BADARG, WORKSPACE, LAUNCH, UNSUPPORTED = 0, -1, -2, -3, -4
P = 0x7F0000001000  # fake device pointers
M, QKV, OUT, G, WS, LEN, BIAS = P, P + 0x10000000, P + 0x20000000, P + 0x30000000, P + 0x60000000, P + 0x70000000, P + 0x78000000
BIG = 1 << 40
NAMES = ("vivit_attention_scoremod_jac_t_f32_workspace_bytes", "vivit_attention_scoremod_jac_t_f32")
INF, NAN = float("inf"), float("nan")
MODS = [(50.0, None), (0.0, BIAS), (0.5, BIAS), (0.0, None)]   # a cap, a table, both, neither (the forwarded call)


def call(V=3, N=2, T=17, H=4, Hkv=2, d=20, M=M, qkv=QKV, out=OUT, G=G, ws=WS, wsb=BIG, causal=0, lengths=LEN, window=5, softcap=50.0,
         bias=BIAS):
    return _lib.load().vivit_attention_scoremod_jac_t_f32(M, qkv, out, G, V, N, T, H, Hkv, d, 0.25, causal, lengths, window, softcap, bias,
                                                          ws, wsb, None)


def need(V=3, N=2, T=17, H=4, Hkv=2, d=20):
    return _lib.load().vivit_attention_scoremod_jac_t_f32_workspace_bytes(V, N, T, H, Hkv, d)


def test_symbols_are_exported_bound_and_declared():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "vivit_hip.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert re.search(r"\b(size_t|int) " + name + r"\(", header), name
    assert re.search(r"int64_t window, float softcap, const float \*bias, void \*workspace", header)
    assert len(_lib.SIGNATURES[NAMES[1]][1]) == 19 and len(_lib.SIGNATURES[NAMES[0]][1]) == 6
    assert re.search(r"\b10 soft cap\b", header)
    assert _lib.ABI_VERSION == 1008 and lib.vivit_hip_abi_version() == 1008   # exports were only added


def test_workspace_is_that_of_the_masked_entry():
    masked = _lib.load().vivit_attention_masked_jac_t_f32_workspace_bytes
    for shape in ((1, 1, 1, 1, 1, 1), (10, 64, 197, 6, 2, 64), (3, 2, 4097, 8, 1, 128), (10, 4, 512, 32, 8, 128), (3, 2, 17, 4, 4, 20)):
        assert need(*shape) == masked(*shape) > 0
    assert need(d=129) == 0 and need(H=4, Hkv=3) == 0


@pytest.mark.parametrize("softcap", [-1.0, -0.0001, -INF, INF, NAN])
def test_a_cap_that_is_negative_or_not_finite_is_refused(softcap):
    for bias in (BIAS, None):
        assert call(softcap=softcap, bias=bias) == BADARG
        assert call(softcap=softcap, bias=bias, ws=None, wsb=0) == BADARG     # (before the workspace is looked at)
        assert call(softcap=softcap, bias=bias, d=129) == BADARG              # (and before the shape is)


@pytest.mark.parametrize("softcap,bias", MODS)
@pytest.mark.parametrize("which", ["M", "qkv", "out", "G"])
def test_null_operands_are_refused(which, softcap, bias):
    assert call(**{which: None}, softcap=softcap, bias=bias) == BADARG
    assert call(**{which: None}, softcap=softcap, bias=bias, lengths=None, window=0) == BADARG


@pytest.mark.parametrize("softcap,bias", MODS)
@pytest.mark.parametrize("which", ["V", "N", "T", "H", "Hkv", "d"])
def test_non_positive_sizes_are_refused(which, softcap, bias):
    assert call(**{which: 0}, softcap=softcap, bias=bias) == BADARG
    assert call(**{which: -1}, softcap=softcap, bias=bias) == BADARG
    assert need(**{which: 0}) == 0 and need(**{which: -1}) == 0


@pytest.mark.parametrize("softcap,bias", MODS)
def test_a_negative_window_and_unequal_groups_are_refused(softcap, bias):
    assert call(window=-1, softcap=softcap, bias=bias) == BADARG
    assert call(window=-1, softcap=softcap, bias=bias, ws=None, wsb=0) == BADARG
    assert call(H=4, Hkv=3, softcap=softcap, bias=bias) == BADARG


@pytest.mark.parametrize("softcap,bias", MODS)
def test_unsupported_shapes_are_refused_before_the_workspace_check(softcap, bias):
    kw = dict(softcap=softcap, bias=bias)
    assert call(d=129, **kw) == UNSUPPORTED
    assert call(d=129, ws=None, wsb=0, **kw) == UNSUPPORTED
    assert call(d=128, wsb=16, **kw) == WORKSPACE   # (d = 128 itself is supported)
    assert call(V=1 << 20, ws=None, wsb=0, **kw) == UNSUPPORTED
    assert call(T=(1 << 31) - 16, ws=None, wsb=0, **kw) == UNSUPPORTED


@pytest.mark.parametrize("softcap,bias", MODS)
@pytest.mark.parametrize("shape", [(3, 2, 17, 4, 2, 20), (1, 1, 1, 2, 1, 1), (10, 64, 197, 6, 3, 64), (3, 2, 65, 3, 1, 128)])
def test_short_workspace_is_refused(shape, softcap, bias):
    want = need(*shape)
    assert want > 0
    V, N, T, H, Hkv, d = shape
    kw = dict(V=V, N=N, T=T, H=H, Hkv=Hkv, d=d, softcap=softcap, bias=bias)
    assert call(wsb=want - 1, **kw) == WORKSPACE
    assert call(ws=None, wsb=want, **kw) == WORKSPACE
    assert call(ws=None, wsb=0, **kw) == WORKSPACE


def test_every_accepted_argument_reaches_the_workspace_check():
    for softcap in (0.0, 1e-30, 0.5, 50.0, 3e38):
        for bias in (None, BIAS, BIAS + 4):   # (the table needs no alignment beyond four bytes)
            for lengths, window, causal in ((None, 0, 0), (LEN, 0, 1), (None, 1, 1), (LEN, 1 << 62, 0)):
                assert call(softcap=softcap, bias=bias, lengths=lengths, window=window, causal=causal, wsb=16) == WORKSPACE
                assert call(softcap=softcap, bias=bias, lengths=lengths, window=window, causal=causal, ws=None, wsb=0) == WORKSPACE


def act(kind=10, param=30.0, V=2, per_v=64, M=M, x=QKV, out=OUT):
    return _lib.load().vivit_act_jac_t_f32(M, x, out, V, per_v, kind, param, None)


@pytest.mark.parametrize("cap", [0.0, -0.0, -1.0, -INF, INF, NAN])
def test_the_softcap_kind_refuses_a_cap_that_is_not_positive_and_finite(cap):
    assert act(param=cap) == BADARG
    assert act(param=cap, V=0) == BADARG and act(param=cap, per_v=0) == BADARG   # (before the empty call returns)


def test_the_softcap_kind_keeps_the_other_refusals():
    assert act(M=None) == BADARG and act(x=None) == BADARG and act(out=None) == BADARG
    assert act(V=-1) == BADARG and act(per_v=-1) == BADARG
    assert act(kind=11) == BADARG and act(kind=11, param=0.0) == BADARG          # the next number is free
    assert act(V=0) == OK and act(per_v=0) == OK                                  # an empty call launches nothing
    assert act(kind=9, param=-1.0, V=0) == OK                                     # (the parameter of another kind is not looked at)
