"""``vivit_attention_jac_t_f32`` (include/vivit_hip.h): the refusing half of the entry point and its workspace query.

No GPU is needed and none is used: every call below must be refused by the host-side checks before anything is enqueued (as
tests/test_symeig_batched_abi.py does for the batched solve; the pointers are fake non-null addresses that the host never
dereferences)."""
import pytest

from vivit_amd import _lib

OK, BADARG, WORKSPACE, LAUNCH, UNSUPPORTED = 0, -1, -2, -3, -4
P = 0x7F0000001000  # fake device pointers
M, QKV, OUT, G, WS = P, P + 0x10000000, P + 0x20000000, P + 0x30000000, P + 0x60000000
BIG = 1 << 40


def call(V=3, N=2, T=17, H=2, d=20, M=M, qkv=QKV, out=OUT, G=G, ws=WS, wsb=BIG, causal=0):
    return _lib.load().vivit_attention_jac_t_f32(M, qkv, out, G, V, N, T, H, d, 0.25, causal, ws, wsb, None)


def need(V=3, N=2, T=17, H=2, d=20):
    return _lib.load().vivit_attention_jac_t_f32_workspace_bytes(V, N, T, H, d)


def test_symbols_are_exported_and_bound():
    lib = _lib.load()
    for name in ("vivit_attention_jac_t_f32", "vivit_attention_jac_t_f32_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.ABI_VERSION == 1008 and lib.vivit_hip_abi_version() == 1008   # exports were only added


def test_workspace_query_is_monotone_in_T_and_linear_in_the_row_statistics():
    sizes = [need(T=T) for T in (1, 5, 16, 17, 33, 65, 197, 1024, 4097)]
    assert sizes[0] > 0 and all(b > a for a, b in zip(sizes, sizes[1:])), sizes
    # the row log-sum-exp [N, H, T] and D [V, N, H, T], nothing of size T x T
    for V, N, T, H, d in ((1, 1, 1, 1, 1), (10, 64, 197, 6, 64), (3, 2, 4097, 2, 128)):
        assert 4 * (V + 1) * N * H * T <= need(V, N, T, H, d) <= 4 * (V + 1) * N * H * T + 256


@pytest.mark.parametrize("which", ["M", "qkv", "out", "G"])
def test_null_pointers_are_refused(which):
    assert call(**{which: None}) == BADARG


@pytest.mark.parametrize("which", ["V", "N", "T", "H", "d"])
def test_non_positive_sizes_are_refused(which):
    assert call(**{which: 0}) == BADARG
    assert call(**{which: -3}) == BADARG
    assert need(**{which: 0}) == 0


def test_unsupported_shapes_are_refused_before_the_workspace_check():
    assert call(d=129) == UNSUPPORTED
    assert call(d=129, ws=None, wsb=0) == UNSUPPORTED
    assert need(d=129) == 0
    assert call(d=128, wsb=16) == WORKSPACE   # (d = 128 itself is supported)
    # element counts beyond the kernels' index arithmetic
    assert call(H=1 << 40, d=1) == UNSUPPORTED
    assert call(N=1 << 31, H=2) == UNSUPPORTED
    assert call(T=(1 << 31) - 16) == UNSUPPORTED
    assert call(V=1 << 50, N=1 << 20, T=1 << 20) == UNSUPPORTED
    assert call(V=1 << 20) == UNSUPPORTED     # factor rows beyond the grid's second dimension


@pytest.mark.parametrize("shape", [(3, 2, 17, 2, 20), (1, 1, 1, 1, 1), (10, 64, 197, 6, 64), (3, 2, 65, 3, 128)])
def test_short_workspace_is_refused(shape):
    want = need(*shape)
    assert want > 0
    V, N, T, H, d = shape
    kw = dict(V=V, N=N, T=T, H=H, d=d)
    assert call(wsb=want - 1, **kw) == WORKSPACE
    assert call(ws=None, wsb=want, **kw) == WORKSPACE
    assert call(ws=None, wsb=0, **kw) == WORKSPACE
