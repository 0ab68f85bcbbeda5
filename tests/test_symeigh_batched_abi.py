"""``vivit_symeig_reduce_batched_f32`` / ``vivit_symeig_select_batched_f32`` (include/vivit_hip.h): the refusing half of
the entry points and the workspace query.

No GPU is needed and none is used: every call below must be refused by the host-side checks before anything is enqueued
(pattern of tests/test_symeig_batched_abi.py; the pointers are fake non-null addresses that the host never dereferences
-- only the HOST arrays are read).  The batched solve has no counterpart in the reference, which solves one group at a
time (vivit/linalg/eigh.py:248-253)."""
import ctypes

import pytest

from vivit_amd import _lib

OK, BADARG, WORKSPACE, LAUNCH, UNSUPPORTED = 0, -1, -2, -3, -4
P = 0x7F0000001000  # fake device pointer
WOUT, INFO, WS, IDX = P + 0x40000000, P + 0x50000000, P + 0x60000000, P + 0x70000000
BIG = 1 << 40


def ptrs(batch, null_at=None, base=P):
    arr = (ctypes.c_void_p * batch)(*[base + 0x1000000 * i for i in range(batch)])
    if null_at is not None:
        arr[null_at] = None
    return arr


def ks(values):
    return (ctypes.c_int64 * len(values))(*values)


def state_need(n):
    return _lib.load().vivit_symeig_reduce_f32_workspace_bytes(n)


def reduce(A, batch, n, lda, W=WOUT, state="default", each=BIG, info=INFO):
    state = ptrs(max(batch, 1), base=P + 0x100000000) if state == "default" else state
    return _lib.load().vivit_symeig_reduce_batched_f32(A, batch, n, lda, W, state, each, info, None)


def select(A, batch, n, lda, K="default", idx=IDX, Zt="default", ldz=None, state="default", each=BIG, ws=WS, wsb=BIG,
           info=INFO):
    nb = max(batch, 1)
    K = ks([10] * nb) if K == "default" else K
    Zt = ptrs(nb, base=P + 0x200000000) if Zt == "default" else Zt
    state = ptrs(nb, base=P + 0x100000000) if state == "default" else state
    return _lib.load().vivit_symeig_select_batched_f32(A, batch, n, lda, idx, K, Zt, n if ldz is None else ldz, state, each,
                                                       ws, wsb, info, None)


def need(n, batch, kmax):
    return _lib.load().vivit_symeig_select_batched_f32_workspace_bytes(n, batch, kmax)


@pytest.mark.parametrize("n", [256, 1024])
def test_reduce_refuses_bad_arguments(n):
    assert reduce(None, 3, n, n) == BADARG                       # null pointer array
    assert reduce(ptrs(3, null_at=1), 3, n, n) == BADARG         # a null matrix in it
    assert reduce(ptrs(3), 0, n, n) == BADARG                    # batch = 0
    assert reduce(ptrs(3), -2, n, n) == BADARG
    assert reduce(ptrs(3), 3, n, n - 1) == BADARG                # lda < n
    assert reduce(ptrs(3), 3, n, n, W=None) == BADARG
    assert reduce(ptrs(3), 3, n, n, info=None) == BADARG
    assert reduce(ptrs(3), 3, n, n, state=None) == BADARG        # null state array
    assert reduce(ptrs(3), 3, 0, 0) == BADARG
    assert reduce(ptrs(3), 3, n, n, each=state_need(n) - 1) == WORKSPACE                     # short state
    assert reduce(ptrs(3), 3, n, n, state=ptrs(3, null_at=2, base=P + 0x100000000)) == WORKSPACE   # a null state block


@pytest.mark.parametrize("n", [256, 1024])
def test_select_refuses_bad_arguments(n):
    assert select(None, 3, n, n) == BADARG
    assert select(ptrs(3, null_at=0), 3, n, n) == BADARG
    assert select(ptrs(3), 0, n, n) == BADARG
    assert select(ptrs(3), -1, n, n) == BADARG
    assert select(ptrs(3), 3, n, n - 1) == BADARG                # lda < n
    assert select(ptrs(3), 3, n, n, ldz=n - 1) == BADARG         # ldz < n
    assert select(ptrs(3), 3, n, n, K=None) == BADARG
    assert select(ptrs(3), 3, n, n, K=ks([10, -1, 10])) == BADARG        # negative K_b
    assert select(ptrs(3), 3, n, n, K=ks([10, n + 1, 10])) == BADARG     # K_b > n
    assert select(ptrs(3), 3, n, n, Zt=None) == BADARG
    assert select(ptrs(3), 3, n, n, Zt=ptrs(3, null_at=1, base=P + 0x200000000)) == BADARG   # rows wanted, no output
    assert select(ptrs(3), 3, n, n, idx=None) == BADARG
    assert select(ptrs(3), 3, n, n, info=None) == BADARG
    assert select(ptrs(3), 3, n, n, state=None) == BADARG
    assert select(ptrs(3), 3, n, n, each=state_need(n) - 1) == WORKSPACE
    assert select(ptrs(3), 3, n, n, state=ptrs(3, null_at=1, base=P + 0x100000000)) == WORKSPACE
    want = need(n, 3, 10)
    assert want > 0
    assert select(ptrs(3), 3, n, n, wsb=want - 1) == WORKSPACE
    assert select(ptrs(3), 3, n, n, ws=None, wsb=want) == WORKSPACE
    assert select(ptrs(3), 3, n, n, ws=None, wsb=0) == WORKSPACE


def test_sizes_outside_the_batched_range_are_unsupported():
    for n in (192, 1281):
        for batch in (1, 8, 11):
            assert reduce(ptrs(batch), batch, n, n, each=0) == UNSUPPORTED            # (before the state check)
            assert select(ptrs(batch), batch, n, n, ws=None, wsb=0, each=0) == UNSUPPORTED   # (before the workspace check)
        assert need(n, 8, 10) == 0


@pytest.mark.parametrize("kmax", [1, 10, 40, 300])
@pytest.mark.parametrize("n", [193, 256, 777, 1024, 1280])
def test_workspace_grows_up_to_eight_problems_and_is_constant_beyond(n, kmax):
    kmax = min(kmax, n)
    sizes = [need(n, b, kmax) for b in range(1, 9)]
    assert all(b > a for a, b in zip(sizes, sizes[1:])), sizes
    for b in (9, 11, 16, 100, 1000):
        assert need(n, b, kmax) == sizes[7]     # waves of eight reuse the slots
    if kmax > 256:   # the single select's scratch (divide & conquer) is part of it
        assert sizes[0] >= _lib.load().vivit_symeig_select_f32_workspace_bytes(n, kmax)
