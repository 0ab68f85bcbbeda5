"""``vivit_symeigvals_batched_f32`` (include/vivit_hip.h): the refusing half of the entry point and its workspace query.

No GPU is needed and none is used: every call below must be refused by the host-side checks before anything is enqueued
(as tests/test_abi_errors.py does for the other entry points; the pointers are fake non-null addresses that the host
never dereferences -- only the HOST array of matrix pointers is read).  The batched solve has no counterpart in the
reference, which solves one group at a time (vivit/linalg/eigvalsh.py:221)."""
import ctypes

import pytest

from vivit_amd import _lib

OK, BADARG, WORKSPACE, LAUNCH, UNSUPPORTED = 0, -1, -2, -3, -4
P = 0x7F0000001000  # fake device pointer
WOUT = P + 0x40000000
INFO = P + 0x50000000
WS = P + 0x60000000
BIG = 1 << 40


def ptrs(batch, null_at=None):
    arr = (ctypes.c_void_p * batch)(*[P + 0x1000000 * i for i in range(batch)])
    if null_at is not None:
        arr[null_at] = None
    return arr


def solve(A, batch, n, lda, W=WOUT, ws=WS, wsb=BIG, info=INFO):
    return _lib.load().vivit_symeigvals_batched_f32(A, batch, n, lda, W, ws, wsb, info, None)


def need(n, batch):
    return _lib.load().vivit_symeigvals_batched_f32_workspace_bytes(n, batch)


def test_abi_version_is_1008():
    assert _lib.ABI_VERSION == 1008 and _lib.load().vivit_hip_abi_version() == 1008


@pytest.mark.parametrize("n", [64, 256, 1024])
def test_bad_arguments_are_refused(n):
    assert solve(None, 3, n, n) == BADARG                       # null pointer array
    assert solve(ptrs(3, null_at=1), 3, n, n) == BADARG         # a null matrix in it
    assert solve(ptrs(3), 0, n, n) == BADARG                    # batch = 0
    assert solve(ptrs(3), -2, n, n) == BADARG
    assert solve(ptrs(3), 3, n, n - 1) == BADARG                # lda < n
    assert solve(ptrs(3), 3, n, n, W=None) == BADARG
    assert solve(ptrs(3), 3, n, n, info=None) == BADARG
    assert solve(ptrs(3), 3, 0, 0) == BADARG


@pytest.mark.parametrize("n", [193, 256, 1024, 1280])
@pytest.mark.parametrize("batch", [1, 3, 8, 11])
def test_short_workspace_is_refused(n, batch):
    want = need(n, batch)
    assert want > 0
    assert solve(ptrs(batch), batch, n, n, wsb=want - 1) == WORKSPACE
    assert solve(ptrs(batch), batch, n, n, ws=None, wsb=want) == WORKSPACE
    assert solve(ptrs(batch), batch, n, n, ws=None, wsb=0) == WORKSPACE


def test_sizes_above_one_xcd_are_unsupported():
    for batch in (1, 8, 11):
        assert solve(ptrs(batch), batch, 1281, 1281) == UNSUPPORTED
        assert solve(ptrs(batch), batch, 4096, 4096, ws=None, wsb=0) == UNSUPPORTED   # (before the workspace check)
    assert need(1281, 8) == 0


@pytest.mark.parametrize("n", [193, 256, 777, 1024, 1280])
def test_workspace_grows_up_to_eight_problems_and_is_constant_beyond(n):
    sizes = [need(n, b) for b in range(1, 9)]
    assert all(b > a for a, b in zip(sizes, sizes[1:])), sizes
    single = _lib.load().vivit_symeig_f32_workspace_bytes(n, 0)
    assert sizes[0] >= single and sizes[7] >= 8 * single
    for b in (9, 11, 16, 100, 1000):
        assert need(n, b) == sizes[7]     # waves of eight reuse the slots


def test_single_workgroup_sizes_need_no_workspace():
    for n in (1, 64, 192):
        for b in (1, 8, 11):
            assert need(n, b) == 0
