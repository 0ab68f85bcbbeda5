"""The entry point of csrc/loss_positions.hip (include/vivit_hip.h): its refusing half.

No GPU is needed and none is used: every call below must be answered by the host-side checks before anything is enqueued (as
tests/test_llama_abi.py does; the pointers are fake non-null addresses that the host never dereferences)."""
import pytest

from vivit_amd import _lib

OK, BADARG, WORKSPACE, LAUNCH, UNSUPPORTED = 0, -1, -2, -3, -4
P = 0x7F0000001000  # fake device pointers
A, B_, C_ = (P + i * 0x10000000 for i in range(3))
BIG = (1 << 31, 1 << 62)
NAME = "vivit_ce_pos_sqrt_hessian_f32"
SIZES = dict(N=3, C=4, L=5, V=2)       # the sampled factor (idx given): V is free


def call(ptrs=(A, B_, C_), layout=1, **kw):
    s = {**SIZES, **kw}
    return getattr(_lib.load(), NAME)(*ptrs, s["N"], s["C"], s["L"], s["V"], layout, 0.5, None)


def test_symbol_is_exported_and_bound():
    lib = _lib.load()
    assert NAME in _lib.SIGNATURES and hasattr(lib, NAME)
    assert getattr(lib, NAME).argtypes == _lib.SIGNATURES[NAME][1] and len(_lib.SIGNATURES[NAME][1]) == 10
    assert _lib.ABI_VERSION == 1008 and lib.vivit_hip_abi_version() == 1008   # an export was only added


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("which", list(SIZES))
def test_any_zero_size_launches_nothing(which, layout):
    assert call(layout=layout, **{which: 0}) == OK
    assert call(layout=layout, **{which: 0}, ptrs=(None, None, None)) == OK     # and reads no pointer
    assert call(layout=layout, **{which: 0}, ptrs=(A, None, C_)) == OK          # exact mode: before V is compared with C L


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("which", list(SIZES))
def test_negative_sizes_are_refused(which, layout):
    assert call(layout=layout, **{which: -1}) == BADARG
    assert call(layout=layout, **{which: -(1 << 40)}) == BADARG
    assert call(layout=layout, **{which: -1}, ptrs=(None, None, None)) == BADARG


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("which", list(SIZES))
def test_sizes_beyond_the_index_arithmetic_are_unsupported(which, layout):
    for big in BIG:
        assert call(layout=layout, **{which: big}) == UNSUPPORTED


@pytest.mark.parametrize("layout", [0, 1])
def test_products_of_sizes_beyond_the_index_arithmetic_are_unsupported(layout):
    assert call(layout=layout, N=1 << 16, L=1 << 15) == UNSUPPORTED                               # N L positions leave 31 bits
    assert call(layout=layout, N=1 << 15, C=1 << 16, L=1 << 15, V=1 << 15) == UNSUPPORTED          # V N C L above 2^60
    assert call(layout=layout, N=1 << 10, C=1 << 20, L=1 << 20, V=1 << 30) == UNSUPPORTED          # V C L alone above 2^60


def test_null_pointers_are_refused():
    assert call(ptrs=(None, B_, C_)) == BADARG          # logits
    assert call(ptrs=(A, B_, None)) == BADARG           # S
    assert call(ptrs=(None, None, None)) == BADARG


@pytest.mark.parametrize("layout", [-1, 2, 7])
def test_an_unknown_layout_is_refused(layout):
    assert call(layout=layout) == BADARG
    assert call(layout=layout, ptrs=(None, None, None)) == BADARG


@pytest.mark.parametrize("layout", [0, 1])
def test_the_exact_factor_needs_v_equal_to_c_times_l(layout):
    for V in (1, 4, 5, 19, 21):                          # C L = 20
        assert call(layout=layout, ptrs=(A, None, C_), V=V) == BADARG
