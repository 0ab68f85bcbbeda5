"""csrc/depthwise.hip: the refusals, all from host-side checks before any launch (no GPU; fake pointers, as tests/test_llama_abi.py)."""
import pytest

from vivit_amd import _lib

BADARG, UNSUPPORTED, PTRS = -1, -4, tuple(0x7F0000001000 + i * 0x10000000 for i in range(3))   # (fake device pointers)
NAMES = ("vivit_dwconv2d_jac_t_f32", "vivit_dwconv2d_weight_mjp_f32")
GEOM = dict(C=4, mult=1, H=5, W=5, KH=3, KW=3, OH=5, OW=5, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1)   # 3 x 3, padding 1, 5 x 5 plane


def call(name, ptrs=PTRS, **kw):
    sizes = {"rows": 4, **({"N": 2} if "weight" in name else {}), **GEOM, **kw}
    return getattr(_lib.load(), name)(*ptrs, *sizes.values(), None)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("bad", [dict(H=-5), dict(rows=-1), dict(C=0), dict(sh=0), dict(dw=0), dict(ph=-1), dict(OH=6), dict(OW=7)] +
                         [dict(ptrs=PTRS[:i] + (None,) + PTRS[i + 1:]) for i in range(3)], ids=str)
def test_bad_arguments_are_refused(name, bad):
    assert call(name, **bad) == BADARG


@pytest.mark.parametrize("name", NAMES)
def test_exported_and_more_than_128_taps_unsupported(name):
    assert name in _lib.SIGNATURES and getattr(_lib.load(), name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.ABI_VERSION == 1008 and _lib.load().vivit_hip_abi_version() == 1008   # exports were only added
    big = dict(H=64, W=64, ph=0, pw=0)
    assert call(name, KH=3, KW=43, OH=62, OW=22, **big) == UNSUPPORTED       # 129 taps
    assert call(name, KH=8, KW=16, OH=57, OW=49, **big, ptrs=(None,) + PTRS[1:]) == BADARG   # 128 taps pass that check
    assert call(name, H=1 << 16, W=1 << 16, OH=1 << 16, OW=1 << 16) == UNSUPPORTED       # a plane of 2^32 elements
