"""The three entry points of the weighted cross-entropy factors (include/vivit_hip.h: ``vivit_ce_target_scales_f32`` with its workspace
query, ``vivit_ce_pos_sqrt_hessian_w_f32``, ``vivit_ce_sqrt_hessian_w_f32``): their refusing half.

No GPU is needed and none is used: every call below must be answered by the host-side checks before anything is enqueued (as
tests/test_loss_positions_abi.py does; the pointers are fake non-null addresses that the host never dereferences)."""
import pytest

from vivit_amd import _lib

OK, BADARG, WORKSPACE, LAUNCH, UNSUPPORTED = 0, -1, -2, -3, -4
P = 0x7F0000001000  # fake device pointers
A, B_, C_, D_, W_ = (P + i * 0x10000000 for i in range(5))
BIG = (1 << 31, 1 << 62)
POS, FLAT, SCALES, QUERY = ("vivit_ce_pos_sqrt_hessian_w_f32", "vivit_ce_sqrt_hessian_w_f32", "vivit_ce_target_scales_f32",
                            "vivit_ce_target_scales_f32_workspace_bytes")
POS_SIZES = dict(N=3, C=4, L=5, V=2)       # the sampled factor (idx given): V is free


def pos(ptrs=(A, B_, C_, D_), layout=1, **kw):
    """ptrs: logits, idx, pos_scale, S."""
    s = {**POS_SIZES, **kw}
    return getattr(_lib.load(), POS)(*ptrs, s["N"], s["C"], s["L"], s["V"], layout, None)


def flat(ptrs=(A, B_, C_, D_), N=3, C=4, V=2):
    """ptrs: logits, onehot, row_scale, S."""
    return getattr(_lib.load(), FLAT)(*ptrs, N, C, V, None)


def scales(ptrs=(A, B_, C_), R=7, C=4, ignore_index=-100, eps=0.1, mean=1, mult=1, ws=W_, ws_bytes=None):
    """ptrs: target, class_weight, pos_scale."""
    lib = _lib.load()
    if ws_bytes is None:
        ws_bytes = getattr(lib, QUERY)(max(R, 0), max(C, 0))
    return getattr(lib, SCALES)(*ptrs, R, C, ignore_index, eps, mean, mult, ws, ws_bytes, None)


def test_symbols_are_exported_and_bound():
    lib = _lib.load()
    for name, nargs in ((POS, 10), (FLAT, 8), (SCALES, 12), (QUERY, 2)):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1] and len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib.ABI_VERSION == 1008 and lib.vivit_hip_abi_version() == 1008   # exports were only added


# ---- the per-position factor ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("which", list(POS_SIZES))
def test_positions_any_zero_size_launches_nothing(which, layout):
    assert pos(layout=layout, **{which: 0}) == OK
    assert pos(layout=layout, **{which: 0}, ptrs=(None, None, None, None)) == OK     # and reads no pointer
    assert pos(layout=layout, **{which: 0}, ptrs=(A, None, C_, D_)) == OK            # exact mode: before V is compared with C L


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("which", list(POS_SIZES))
def test_positions_negative_sizes_are_refused(which, layout):
    assert pos(layout=layout, **{which: -1}) == BADARG
    assert pos(layout=layout, **{which: -(1 << 40)}) == BADARG
    assert pos(layout=layout, **{which: -1}, ptrs=(None, None, None, None)) == BADARG


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("which", list(POS_SIZES))
def test_positions_sizes_beyond_the_index_arithmetic_are_unsupported(which, layout):
    for big in BIG:
        assert pos(layout=layout, **{which: big}) == UNSUPPORTED


@pytest.mark.parametrize("layout", [0, 1])
def test_positions_products_of_sizes_beyond_the_index_arithmetic_are_unsupported(layout):
    assert pos(layout=layout, N=1 << 16, L=1 << 15) == UNSUPPORTED                               # N L positions leave 31 bits
    assert pos(layout=layout, N=1 << 15, C=1 << 16, L=1 << 15, V=1 << 15) == UNSUPPORTED          # V N C L above 2^60
    assert pos(layout=layout, N=1 << 10, C=1 << 20, L=1 << 20, V=1 << 30) == UNSUPPORTED          # V C L alone above 2^60


def test_positions_null_pointers_are_refused():
    assert pos(ptrs=(None, B_, C_, D_)) == BADARG       # logits
    assert pos(ptrs=(A, B_, None, D_)) == BADARG        # pos_scale
    assert pos(ptrs=(A, B_, C_, None)) == BADARG        # S
    assert pos(ptrs=(None, None, None, None)) == BADARG


@pytest.mark.parametrize("layout", [-1, 2, 7])
def test_positions_an_unknown_layout_is_refused(layout):
    assert pos(layout=layout) == BADARG
    assert pos(layout=layout, ptrs=(None, None, None, None)) == BADARG


@pytest.mark.parametrize("layout", [0, 1])
def test_positions_the_exact_factor_needs_v_equal_to_c_times_l(layout):
    for V in (1, 4, 5, 19, 21):                          # C L = 20
        assert pos(layout=layout, ptrs=(A, None, C_, D_), V=V) == BADARG


# ---- the [N, C] factor: the rules of vivit_ce_sqrt_hessian_f32 ----------------------------------------------------------------------------
def test_flat_refusals():
    assert flat(N=0) == OK and flat(N=0, ptrs=(None, None, None, None)) == OK
    for kw in (dict(N=-1), dict(C=0), dict(C=-1), dict(V=0), dict(V=-1)):
        assert flat(**kw) == BADARG
    assert flat(ptrs=(None, B_, C_, D_)) == BADARG      # logits
    assert flat(ptrs=(A, B_, None, D_)) == BADARG       # row_scale
    assert flat(ptrs=(A, B_, C_, None)) == BADARG       # S
    assert flat(ptrs=(A, None, C_, D_), V=3) == BADARG  # exact: V must equal C
    assert flat(C=15361) == UNSUPPORTED                 # the classes of a sample no longer fit the workgroup's LDS
    assert flat(N=1 << 31) == UNSUPPORTED


# ---- the scales ------------------------------------------------------------------------------------------------------------------------
def test_scales_workspace_query():
    q = getattr(_lib.load(), QUERY)
    assert q(7, 4) > 0 and q(7, 4) % 8 == 0
    assert q(1 << 30, 1 << 20) == q(7, 4)               # (a fixed number of partial sums)


def test_scales_zero_rows_launch_nothing():
    assert scales(R=0) == OK
    assert scales(R=0, ptrs=(None, None, None), ws=None, ws_bytes=0) == OK
    assert scales(R=0, C=0) == OK


def test_scales_bad_arguments_are_refused():
    assert scales(R=-1) == BADARG and scales(C=-1) == BADARG
    assert scales(R=-1, ptrs=(None, None, None)) == BADARG
    assert scales(mult=0) == BADARG and scales(mult=-3) == BADARG
    assert scales(mean=2) == BADARG and scales(mean=-1) == BADARG
    assert scales(ptrs=(None, B_, C_)) == BADARG        # target
    assert scales(ptrs=(A, B_, None)) == BADARG         # pos_scale
    for big in BIG:
        assert scales(R=big) == UNSUPPORTED and scales(C=big) == UNSUPPORTED and scales(mult=big) == UNSUPPORTED


def test_scales_workspace_is_checked():
    need = getattr(_lib.load(), QUERY)(7, 4)
    assert scales(ws=None) == WORKSPACE
    assert scales(ws_bytes=need - 1) == WORKSPACE and scales(ws_bytes=0) == WORKSPACE
    assert scales(ws=W_ + 4) == WORKSPACE               # fp64 partial sums: 8-byte alignment
