"""``vivit_attention_wide_forward_f32``, ``vivit_attention_wide_backward_f32`` and its workspace query (include/vivit_hip.h): the
refusing half, and the bound of the GPU test on its own cases.  No GPU is needed and none is used: every call is refused by the
host-side checks before anything is enqueued (the pointers are fake non-null addresses that the host never dereferences, as in
tests/test_attention_backward_abi.py).

On the commit before the feature this whole file fails: the symbols do not exist."""
import pytest

import attention_forward_refs as fr
import attention_scoremod_refs as sr
import test_attention_wide_fused_gpu as cases
from vivit_amd import _lib

BADARG, UNSUPPORTED, WORKSPACE = -1, -4, -2
P = 0x7F0000001000  # fake device pointers
DOUT, QKV, OUT, LSE, DQ, LEN, BIAS, WS = (P + k * 0x10000000 for k in range(8))


def ws_query(N=2, T=17, H=4, Hkv=2, d=192):
    return _lib.load().vivit_attention_wide_backward_f32_workspace_bytes(N, T, H, Hkv, d)


def forward(N=2, T=17, H=4, Hkv=2, d=192, qkv=QKV, out=OUT, lse=LSE, window=5, softcap=1.5, bias=BIAS, **_):
    return _lib.load().vivit_attention_wide_forward_f32(qkv, out, lse, N, T, H, Hkv, d, 0.25, 1, LEN, window, softcap, bias, None)


def backward(N=2, T=17, H=4, Hkv=2, d=192, dout=DOUT, qkv=QKV, out=OUT, lse=LSE, dqkv=DQ, window=5, softcap=1.5, bias=BIAS, ws=WS,
             ws_bytes=None):
    ws_bytes = ws_query(N, T, H, Hkv, d) if ws_bytes is None else ws_bytes
    return _lib.load().vivit_attention_wide_backward_f32(dout, qkv, out, lse, dqkv, N, T, H, Hkv, d, 0.25, 1, LEN, window, softcap, bias,
                                                         ws, ws_bytes, None)


def test_the_workspace_is_d_alone_and_zero_for_refused_arguments():
    assert ws_query() == 2 * 4 * 17 * 4   # D [N, H, T] floats
    for kw in (dict(d=16), dict(d=128), dict(d=257), dict(d=512), dict(N=0), dict(H=4, Hkv=3), dict(d=-1), dict(T=(1 << 31) - 16)):
        assert ws_query(**kw) == 0, kw
    assert _lib.load().vivit_hip_abi_version() == 1008   # exports were only added


@pytest.mark.parametrize("entry", [forward, backward])
@pytest.mark.parametrize("softcap,bias", [(1.5, BIAS), (0.0, None)])
def test_refusals_follow_the_order_of_the_narrow_entries(entry, softcap, bias):
    kw = dict(softcap=softcap, bias=bias)
    for d in (16, 128, 257, 512):   # before the workspace is looked at
        assert entry(d=d, ws=None, ws_bytes=0, **kw) == UNSUPPORTED
    for bad in (-1.0, float("inf"), float("nan")):   # the cap first: before the operands and the shape
        assert entry(softcap=bad, bias=bias, qkv=None, d=128) == BADARG
    for which in ("qkv", "out") + (("dout", "lse", "dqkv") if entry is backward else ()):
        assert entry(**{which: None}, d=128, **kw) == BADARG
    assert entry(window=-1, d=128, **kw) == BADARG
    for which in ("N", "T", "H", "Hkv", "d"):
        assert entry(**{which: 0}, **kw) == BADARG and entry(**{which: -1}, **kw) == BADARG
    assert entry(H=4, Hkv=3, **kw) == BADARG
    assert entry(T=(1 << 31) - 16, **kw) == UNSUPPORTED and entry(N=1 << 31, **kw) == UNSUPPORTED
    if entry is backward:
        assert entry(ws=None, **kw) == WORKSPACE and entry(ws_bytes=ws_query() - 1, **kw) == WORKSPACE


def test_the_ctypes_wrappers_raise_on_d_128():
    """(``kernels.attention_wide_forward`` itself takes device tensors only: tests/test_attention_wide_fused_gpu.py asks it.)"""
    for name, entry in (("vivit_attention_wide_forward_f32", forward), ("vivit_attention_wide_backward_f32", backward)):
        assert name in _lib.SIGNATURES
        with pytest.raises(_lib.VivitHipError, match=name) as err:
            _lib.check(entry(d=128), name)
        assert err.value.status == _lib.VIVIT_E_UNSUPPORTED


@pytest.mark.parametrize("case", range(len(cases.CASES)), ids=cases.IDS)
def test_the_bound_admits_the_torch_formula_in_fp32(case):
    """The torch formula in fp32 on the CPU lies within ``fr.self_forward``'s bound of the fp64 result at these widths."""
    _, _, H, Hkv, _, _ = cases.CASES[case]
    _, qkv, scale, table = cases.operands(case)
    ref_out, e_out, _, _ = fr.self_forward(qkv, H, Hkv, scale, *cases.mod_args(case), table)
    ok, msg = fr.within(sr.forward(qkv, H, Hkv, scale, *cases.mod_args(case), table), ref_out, e_out)
    assert ok, msg
