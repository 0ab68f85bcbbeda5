"""The entry point of csrc/seq_linear.hip (include/vivit_hip.h): its refusing half.

No GPU is needed and none is used: every call below must be answered by the host-side checks before anything is enqueued (as
tests/test_embedding_abi.py does; the pointers are fake non-null addresses that the host never dereferences)."""
import pytest

from vivit_amd import _lib

OK, BADARG, WORKSPACE, LAUNCH, UNSUPPORTED = 0, -1, -2, -3, -4
P = 0x7F0000001000  # fake device pointers
A, B_, C = P, P + 0x10000000, P + 0x20000000
SIZES = dict(Cr=2, Nr=3, Cc=3, Nc=5, T=4)
NAME = "vivit_gram_seq_reduce_f32"


def call(p=(A, B_, C), ldz=None, lds=None, ldg=None, **kw):
    s = {**SIZES, **kw}
    ldz = s["Nc"] * s["T"] if ldz is None else ldz
    lds = s["Cc"] * s["Nc"] * s["T"] if lds is None else lds
    ldg = s["Cc"] * s["Nc"] if ldg is None else ldg
    return _lib.load().vivit_gram_seq_reduce_f32(p[0], ldz, p[1], lds, p[2], ldg, s["Cr"], s["Nr"], s["Cc"], s["Nc"], s["T"], 1.0, 0.0, None)


def test_symbol_is_exported_and_bound():
    lib = _lib.load()
    assert NAME in _lib.SIGNATURES and hasattr(lib, NAME)
    assert getattr(lib, NAME).argtypes == _lib.SIGNATURES[NAME][1] and len(_lib.SIGNATURES[NAME][1]) == 14
    assert _lib.ABI_VERSION == 1008 and lib.vivit_hip_abi_version() == 1008   # an export was only added


@pytest.mark.parametrize("which", range(3))
def test_null_pointers_are_refused(which):
    ptrs = (A, B_, C)
    assert call(p=ptrs[:which] + (None,) + ptrs[which + 1:]) == BADARG


@pytest.mark.parametrize("which", list(SIZES))
def test_negative_sizes_are_refused(which):
    assert call(**{which: -1}, ldz=64, lds=64, ldg=64) == BADARG
    assert call(**{which: -(1 << 40)}, ldz=64, lds=64, ldg=64) == BADARG
    assert call(**{which: -1}, p=(None, None, None), ldz=64, lds=64, ldg=64) == BADARG


def test_short_leading_dimensions_are_refused():
    assert call(ldz=5 * 4 - 1) == BADARG
    assert call(lds=3 * 5 * 4 - 1) == BADARG
    assert call(ldg=3 * 5 - 1) == BADARG
    assert call(ldz=0) == BADARG and call(lds=-1) == BADARG and call(ldg=-5) == BADARG


@pytest.mark.parametrize("which", list(SIZES))
def test_any_zero_size_launches_nothing(which):
    assert call(**{which: 0}) == OK
    assert call(**{which: 0}, p=(None, None, None)) == OK                      # and reads no pointer
    assert call(**{which: 0}, ldz=1 << 20, lds=1 << 20, ldg=1 << 20) == OK


def test_all_zero_with_zero_leading_dimensions():
    assert call(Cr=0, Nr=0, Cc=0, Nc=0, T=0, ldz=0, lds=0, ldg=0, p=(None, None, None)) == OK


def test_sizes_beyond_the_index_arithmetic_are_unsupported():
    big = dict(ldz=1 << 62, lds=1 << 62, ldg=1 << 62)
    for which in SIZES:
        assert call(**{which: 1 << 31}, **big) == UNSUPPORTED
        assert call(**{which: 1 << 62}, **big) == UNSUPPORTED
    assert call(T=1025, **big) == UNSUPPORTED                                  # a T x T block is summed by one workgroup
    assert call(Cr=1 << 16, Nr=1 << 15, **big) == UNSUPPORTED                  # Cr Nr leaves 31 bits
    assert call(Cc=1 << 16, Nc=1 << 15, **big) == UNSUPPORTED
    assert call(Cr=1 << 10, Nr=1 << 10, T=1 << 11, **big) == UNSUPPORTED       # (c, n, t) leaves 31 bits
    assert call(Cc=1 << 14, Nc=1 << 14, T=8, **big) == UNSUPPORTED             # (e, m, u) leaves 31 bits
    ok = dict(Cc=1, Nc=8, T=4)
    assert call(**ok, ldz=1 << 31) == UNSUPPORTED and call(**ok, lds=1 << 31) == UNSUPPORTED and call(**ok, ldg=1 << 31) == UNSUPPORTED
    # one workgroup of 256 lanes per row: 2^24 rows would leave the grid's first dimension (2^24 - 1 is checked on the device)
    assert call(Cr=1 << 12, Nr=1 << 12, Cc=1, Nc=2, T=2, ldz=4, lds=4, ldg=2) == UNSUPPORTED
    # column spans beyond the grid's second dimension: T = 1024 has one output per span
    assert call(Cr=1, Nr=1, Cc=1, Nc=65536, T=1024, ldz=1 << 26, lds=1 << 26, ldg=1 << 16) == UNSUPPORTED
    # a refusal for size comes before the null-pointer check only where no pointer would be read anyway
    assert call(T=1025, p=(None, None, None), **big) in (UNSUPPORTED, BADARG)
