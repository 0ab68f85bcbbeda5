"""``vivit_attention_cross_jac_t_f32`` and its workspace query (include/vivit_hip.h): the refusing half of the entry point.

No GPU is needed and none is used: every call below must be refused by the host-side checks before anything is enqueued (as
tests/test_attention_masked_abi.py does for the masked entry point; the pointers are fake non-null addresses that the host never
dereferences)."""
import os
import re

import pytest

from vivit_amd import _lib

OK, BADARG, WORKSPACE, LAUNCH, UNSUPPORTED = 0, -1, -2, -3, -4
P = 0x7F0000001000  # fake device pointers
M, Q, KV, OUT, GQ, GKV, WS, QLEN, KLEN = (P + i * 0x10000000 for i in range(9))
BIG = 1 << 40
NAMES = ("vivit_attention_cross_jac_t_f32_workspace_bytes", "vivit_attention_cross_jac_t_f32")


def call(V=3, N=2, Tq=17, Tk=29, H=4, Hkv=2, d=20, M=M, q=Q, kv=KV, out=OUT, Gq=GQ, Gkv=GKV, ws=WS, wsb=BIG, qlen=QLEN, klen=KLEN):
    return _lib.load().vivit_attention_cross_jac_t_f32(M, q, kv, out, Gq, Gkv, V, N, Tq, Tk, H, Hkv, d, 0.25, qlen, klen, ws, wsb, None)


def need(V=3, N=2, Tq=17, Tk=29, H=4, Hkv=2, d=20):
    return _lib.load().vivit_attention_cross_jac_t_f32_workspace_bytes(V, N, Tq, Tk, H, Hkv, d)


def test_symbols_are_exported_bound_and_declared():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "vivit_hip.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert re.search(r"\b(size_t|int) " + name + r"\(", header), name
    assert re.search(r"const int32_t \*q_lengths, const int32_t \*k_lengths, void \*workspace", header)
    assert re.search(r"NO causal flag and NO window", header)
    assert _lib.ABI_VERSION == 1008 and lib.vivit_hip_abi_version() == 1008   # exports were only added


def test_workspace_is_that_of_the_grouped_query_entry_on_the_queries():
    gqa = _lib.load().vivit_attention_gqa_jac_t_f32_workspace_bytes
    for V, N, Tq, H, Hkv, d in ((1, 1, 1, 1, 1, 1), (10, 64, 197, 6, 2, 64), (3, 2, 4097, 8, 1, 128), (10, 4, 128, 32, 8, 128), (3, 2, 17, 4, 4, 20)):
        sizes = {need(V, N, Tq, Tk, H, Hkv, d) for Tk in (1, 31, 32, 33, Tq, 1536, 100000)}
        assert sizes == {gqa(V, N, Tq, H, Hkv, d)} and 0 not in sizes
    assert need(d=129) == 0 and need(H=4, Hkv=3) == 0


@pytest.mark.parametrize("which", ["M", "q", "kv", "out"])
def test_null_operands_are_refused(which):
    assert call(**{which: None}) == BADARG
    assert call(**{which: None}, qlen=None, klen=None) == BADARG
    assert call(**{which: None}, ws=None, wsb=0) == BADARG


def test_both_results_null_is_refused_and_either_alone_is_accepted():
    assert call(Gq=None, Gkv=None) == BADARG
    assert call(Gq=None, Gkv=None, ws=None, wsb=0) == BADARG
    # one result alone passes every check up to the workspace test
    for kw in (dict(Gq=None), dict(Gkv=None), dict()):
        assert call(wsb=16, **kw) == WORKSPACE
        assert call(ws=None, wsb=0, **kw) == WORKSPACE


@pytest.mark.parametrize("which", ["V", "N", "Tq", "Tk", "H", "Hkv", "d"])
def test_non_positive_sizes_are_refused(which):
    assert call(**{which: 0}) == BADARG
    assert call(**{which: -1}) == BADARG
    assert need(**{which: 0}) == 0 and need(**{which: -1}) == 0


def test_head_counts_that_do_not_divide_are_refused():
    assert call(H=4, Hkv=3) == BADARG and call(H=2, Hkv=4) == BADARG
    assert call(H=4, Hkv=3, ws=None, wsb=0) == BADARG
    assert need(H=4, Hkv=3) == 0


def test_unsupported_shapes_are_refused_before_the_workspace_check():
    assert call(d=129) == UNSUPPORTED
    assert call(d=129, ws=None, wsb=0) == UNSUPPORTED
    assert call(d=128, wsb=16) == WORKSPACE   # (d = 128 itself is supported)
    # the chunk limit: 65535 chunks of 4 (d <= 32) or 2 (d > 32) factor rows
    assert call(V=1 << 20, ws=None, wsb=0) == UNSUPPORTED and need(V=1 << 20) == 0
    assert call(V=4 * 65535, N=1, Tq=1, Tk=1, H=1, Hkv=1, d=1, wsb=16) == WORKSPACE
    assert call(V=4 * 65535 + 1, N=1, Tq=1, Tk=1, H=1, Hkv=1, d=1, ws=None, wsb=0) == UNSUPPORTED
    # 32-bit index arithmetic: either sequence length, either block count, the pitches, the row-dot grid
    assert call(Tq=(1 << 31) - 16, ws=None, wsb=0) == UNSUPPORTED and need(Tq=(1 << 31) - 16) == 0
    assert call(Tk=(1 << 31) - 16, ws=None, wsb=0) == UNSUPPORTED and need(Tk=(1 << 31) - 16) == 0
    assert call(V=1, N=1 << 20, Tq=1, Tk=1 << 20, H=1, Hkv=1, d=1, ws=None, wsb=0) == UNSUPPORTED      # N Hkv ceil(Tk / 32)
    assert call(V=1, N=1 << 20, Tq=1 << 20, Tk=1, H=1, Hkv=1, d=1, ws=None, wsb=0) == UNSUPPORTED      # N H ceil(Tq / 32)
    assert call(V=1, N=1, Tq=1, Tk=1, H=1 << 24, Hkv=1 << 24, d=64, ws=None, wsb=0) == UNSUPPORTED       # the pitches
    assert call(V=60000, N=1 << 10, Tq=1 << 10, Tk=1, H=16, Hkv=1, d=1, ws=None, wsb=0) == UNSUPPORTED   # V N H Tq / 256
    assert need(V=1, N=1 << 20, Tq=1, Tk=1 << 20, H=1, Hkv=1, d=1) == 0


@pytest.mark.parametrize("shape", [(3, 2, 17, 29, 4, 2, 20), (1, 1, 1, 1, 2, 1, 1), (10, 64, 197, 50, 6, 3, 64), (3, 2, 65, 161, 3, 1, 128)])
def test_short_workspace_is_refused(shape):
    want = need(*shape)
    assert want > 0
    V, N, Tq, Tk, H, Hkv, d = shape
    kw = dict(V=V, N=N, Tq=Tq, Tk=Tk, H=H, Hkv=Hkv, d=d)
    assert call(wsb=want - 1, **kw) == WORKSPACE
    assert call(ws=None, wsb=want, **kw) == WORKSPACE
    assert call(ws=None, wsb=0, **kw) == WORKSPACE


def test_every_accepted_lengths_argument_reaches_the_workspace_check():
    for qlen, klen in ((None, None), (QLEN, None), (None, KLEN), (QLEN, KLEN)):
        assert call(qlen=qlen, klen=klen, wsb=16) == WORKSPACE, (qlen, klen)
        assert call(qlen=qlen, klen=klen, ws=None, wsb=0) == WORKSPACE
