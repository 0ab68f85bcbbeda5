"""``vivit_attention_gqa_jac_t_f32``, its workspace query and ``vivit_rope_gqa_jac_t_f32`` (include/vivit_hip.h): the refusing half
of the entry points.

No GPU is needed and none is used: every call below must be refused by the host-side checks before anything is enqueued (as
tests/test_attention_abi.py does for the multi-head entry point; the pointers are fake non-null addresses that the host never
dereferences)."""
import os
import re

import pytest

from vivit_amd import _lib

OK, BADARG, WORKSPACE, LAUNCH, UNSUPPORTED = 0, -1, -2, -3, -4
P = 0x7F0000001000  # fake device pointers
M, QKV, OUT, G, WS = P, P + 0x10000000, P + 0x20000000, P + 0x30000000, P + 0x60000000
BIG = 1 << 40
NAMES = ("vivit_attention_gqa_jac_t_f32_workspace_bytes", "vivit_attention_gqa_jac_t_f32", "vivit_rope_gqa_jac_t_f32")


def call(V=3, N=2, T=17, H=4, Hkv=2, d=20, M=M, qkv=QKV, out=OUT, G=G, ws=WS, wsb=BIG, causal=0):
    return _lib.load().vivit_attention_gqa_jac_t_f32(M, qkv, out, G, V, N, T, H, Hkv, d, 0.25, causal, ws, wsb, None)


def need(V=3, N=2, T=17, H=4, Hkv=2, d=20):
    return _lib.load().vivit_attention_gqa_jac_t_f32_workspace_bytes(V, N, T, H, Hkv, d)


def rope(R=3, T=5, H=4, Hkv=2, d=4, M=M, cos=QKV, sin=OUT, G=G):
    return _lib.load().vivit_rope_gqa_jac_t_f32(M, cos, sin, G, R, T, H, Hkv, d, None)


def test_symbols_are_exported_bound_and_declared():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "vivit_hip.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert re.search(r"\b(size_t|int) " + name + r"\(", header), name
    assert _lib.ABI_VERSION == 1008 and lib.vivit_hip_abi_version() == 1008   # exports were only added


def test_workspace_is_counted_in_query_heads():
    # the row log-sum-exp [N, H, T] and D [V, N, H, T], nothing of size T x T and nothing per key / value head
    for V, N, T, H, Hkv, d in ((1, 1, 1, 1, 1, 1), (10, 64, 197, 6, 2, 64), (3, 2, 4097, 8, 1, 128), (10, 4, 512, 32, 8, 128)):
        assert 4 * (V + 1) * N * H * T <= need(V, N, T, H, Hkv, d) <= 4 * (V + 1) * N * H * T + 256
        assert need(V, N, T, H, Hkv, d) == need(V, N, T, H, H, d) == _lib.load().vivit_attention_jac_t_f32_workspace_bytes(V, N, T, H, d)


@pytest.mark.parametrize("which", ["M", "qkv", "out", "G"])
def test_null_pointers_are_refused(which):
    assert call(**{which: None}) == BADARG


@pytest.mark.parametrize("which", ["V", "N", "T", "H", "Hkv", "d"])
def test_non_positive_sizes_are_refused(which):
    assert call(**{which: 0}) == BADARG
    assert call(**{which: -1}) == BADARG
    assert need(**{which: 0}) == 0 and need(**{which: -1}) == 0


def test_head_counts_that_do_not_divide_are_refused():
    assert call(H=4, Hkv=3) == BADARG and need(H=4, Hkv=3) == 0
    assert call(H=2, Hkv=4) == BADARG
    assert call(H=4, Hkv=3, ws=None, wsb=0) == BADARG            # (before the workspace is looked at)
    for Hkv in (1, 2, 4):
        assert call(H=4, Hkv=Hkv, wsb=16) == WORKSPACE          # (these are supported)


def test_unsupported_shapes_are_refused_before_the_workspace_check():
    assert call(d=129) == UNSUPPORTED
    assert call(d=129, ws=None, wsb=0) == UNSUPPORTED
    assert need(d=129) == 0
    assert call(d=128, wsb=16) == WORKSPACE   # (d = 128 itself is supported)
    # the row pitch (H + 2 Hkv) d beyond 2^31 - 1: 3 H d is, H d alone is not
    H = 1 << 23
    assert H * 128 < 2 ** 31 - 1 < (H + 2 * H) * 128
    assert call(H=H, Hkv=1, d=128, wsb=16) == WORKSPACE       # ((H + 2) d is within the range: supported)
    assert call(H=H, Hkv=H, d=128, ws=None, wsb=0) == UNSUPPORTED
    assert (H + 2 * (H >> 1)) * 128 > 2 ** 31 - 1 and call(H=H, Hkv=H >> 1, d=128, ws=None, wsb=0) == UNSUPPORTED
    assert call(H=1 << 40, Hkv=1, d=1, ws=None, wsb=0) == UNSUPPORTED
    # the block counts N H KB and N Hkv KB beyond 2^31 - 1
    assert call(N=1 << 31, H=2, Hkv=1, ws=None, wsb=0) == UNSUPPORTED
    assert call(N=1 << 20, T=1 << 20, H=4, Hkv=4, d=1, ws=None, wsb=0) == UNSUPPORTED
    assert call(N=1 << 20, T=1 << 20, H=4, Hkv=1, d=1, ws=None, wsb=0) == UNSUPPORTED
    assert call(T=(1 << 31) - 16, ws=None, wsb=0) == UNSUPPORTED
    assert call(V=1 << 50, N=1 << 20, T=1 << 20, ws=None, wsb=0) == UNSUPPORTED
    assert call(V=1 << 20, ws=None, wsb=0) == UNSUPPORTED     # factor rows beyond the grid's second dimension


@pytest.mark.parametrize("shape", [(3, 2, 17, 4, 2, 20), (1, 1, 1, 2, 1, 1), (10, 64, 197, 6, 3, 64), (3, 2, 65, 3, 1, 128)])
def test_short_workspace_is_refused(shape):
    want = need(*shape)
    assert want > 0
    V, N, T, H, Hkv, d = shape
    kw = dict(V=V, N=N, T=T, H=H, Hkv=Hkv, d=d)
    assert call(wsb=want - 1, **kw) == WORKSPACE
    assert call(ws=None, wsb=want, **kw) == WORKSPACE
    assert call(ws=None, wsb=0, **kw) == WORKSPACE


def test_rotary_entry_point_refuses():
    assert rope(Hkv=0) == BADARG and rope(Hkv=-1) == BADARG and rope(H=4, Hkv=3) == BADARG
    assert rope(d=3) == BADARG and rope(R=-1) == BADARG
    for which in ("M", "cos", "sin", "G"):
        assert rope(**{which: None}) == BADARG
    assert rope(R=0) == OK and rope(T=0) == OK and rope(d=0) == OK        # nothing to do, nothing launched
    assert rope(H=1 << 23, Hkv=1 << 23, d=128) == UNSUPPORTED             # (H + 2 Hkv) d beyond 2^31 - 1
    assert rope(R=1 << 20, T=1 << 20) == UNSUPPORTED
