"""``vivit_attention_masked_jac_t_f32`` and its workspace query (include/vivit_hip.h): the refusing half of the entry point.

No GPU is needed and none is used: every call below must be refused by the host-side checks before anything is enqueued (as
tests/test_attention_gqa_abi.py does for the grouped-query entry point; the pointers are fake non-null addresses that the host never
dereferences)."""
import os
import re

import pytest

from vivit_amd import _lib

OK, BADARG, WORKSPACE, LAUNCH, UNSUPPORTED = 0, -1, -2, -3, -4
P = 0x7F0000001000  # fake device pointers
M, QKV, OUT, G, WS, LEN = P, P + 0x10000000, P + 0x20000000, P + 0x30000000, P + 0x60000000, P + 0x70000000
BIG = 1 << 40
NAMES = ("vivit_attention_masked_jac_t_f32_workspace_bytes", "vivit_attention_masked_jac_t_f32")


def call(V=3, N=2, T=17, H=4, Hkv=2, d=20, M=M, qkv=QKV, out=OUT, G=G, ws=WS, wsb=BIG, causal=0, lengths=LEN, window=5):
    return _lib.load().vivit_attention_masked_jac_t_f32(M, qkv, out, G, V, N, T, H, Hkv, d, 0.25, causal, lengths, window, ws, wsb, None)


def need(V=3, N=2, T=17, H=4, Hkv=2, d=20):
    return _lib.load().vivit_attention_masked_jac_t_f32_workspace_bytes(V, N, T, H, Hkv, d)


def test_symbols_are_exported_bound_and_declared():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "vivit_hip.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert re.search(r"\b(size_t|int) " + name + r"\(", header), name
    assert re.search(r"const int32_t \*lengths,\s+int64_t window, void \*workspace", header)
    assert _lib.ABI_VERSION == 1008 and lib.vivit_hip_abi_version() == 1008   # exports were only added


def test_workspace_is_that_of_the_grouped_query_entry():
    gqa = _lib.load().vivit_attention_gqa_jac_t_f32_workspace_bytes
    for shape in ((1, 1, 1, 1, 1, 1), (10, 64, 197, 6, 2, 64), (3, 2, 4097, 8, 1, 128), (10, 4, 512, 32, 8, 128), (3, 2, 17, 4, 4, 20)):
        assert need(*shape) == gqa(*shape) > 0
    assert need(d=129) == 0 and need(H=4, Hkv=3) == 0


@pytest.mark.parametrize("which", ["M", "qkv", "out", "G"])
def test_null_operands_are_refused(which):
    assert call(**{which: None}) == BADARG
    assert call(**{which: None}, lengths=None, window=0) == BADARG


@pytest.mark.parametrize("which", ["V", "N", "T", "H", "Hkv", "d"])
def test_non_positive_sizes_are_refused(which):
    assert call(**{which: 0}) == BADARG
    assert call(**{which: -1}) == BADARG
    assert need(**{which: 0}) == 0 and need(**{which: -1}) == 0


def test_a_negative_window_is_refused():
    assert call(window=-1) == BADARG
    assert call(window=-1, lengths=None) == BADARG
    assert call(window=-1, ws=None, wsb=0) == BADARG                 # (before the workspace is looked at)
    assert call(window=-(1 << 40)) == BADARG
    assert call(H=4, Hkv=3) == BADARG


def test_unsupported_shapes_are_refused_before_the_workspace_check():
    assert call(d=129) == UNSUPPORTED
    assert call(d=129, ws=None, wsb=0) == UNSUPPORTED
    assert call(d=128, wsb=16) == WORKSPACE   # (d = 128 itself is supported)
    assert call(V=1 << 20, ws=None, wsb=0) == UNSUPPORTED
    assert call(T=(1 << 31) - 16, ws=None, wsb=0) == UNSUPPORTED


@pytest.mark.parametrize("shape", [(3, 2, 17, 4, 2, 20), (1, 1, 1, 2, 1, 1), (10, 64, 197, 6, 3, 64), (3, 2, 65, 3, 1, 128)])
def test_short_workspace_is_refused(shape):
    want = need(*shape)
    assert want > 0
    V, N, T, H, Hkv, d = shape
    kw = dict(V=V, N=N, T=T, H=H, Hkv=Hkv, d=d)
    assert call(wsb=want - 1, **kw) == WORKSPACE
    assert call(ws=None, wsb=want, **kw) == WORKSPACE
    assert call(ws=None, wsb=0, **kw) == WORKSPACE


def test_every_accepted_mask_argument_reaches_the_workspace_check():
    # null lengths with no window (the call of the two older entry points), either alone, and windows of T, beyond T and beyond an int
    for lengths, window in ((None, 0), (LEN, 0), (None, 1), (LEN, 17), (None, 22), (LEN, (1 << 31) - 1), (None, 1 << 31), (LEN, 1 << 62)):
        assert call(lengths=lengths, window=window, wsb=16) == WORKSPACE, (lengths, window)
        assert call(lengths=lengths, window=window, ws=None, wsb=0) == WORKSPACE
