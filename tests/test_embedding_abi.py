"""The entry points of csrc/embedding.hip (include/vivit_hip.h): the refusing half of each and of the workspace query.

No GPU is needed and none is used: every call below must be refused by the host-side checks before anything is enqueued (as
tests/test_attention_abi.py does; the pointers are fake non-null addresses that the host never dereferences)."""
import pytest

from vivit_amd import _lib

OK, BADARG, WORKSPACE, LAUNCH, UNSUPPORTED = 0, -1, -2, -3, -4
P = 0x7F0000001000  # fake device pointers
A, B_, C, D_, E = P, P + 0x10000000, P + 0x20000000, P + 0x30000000, P + 0x40000000
WS = P + 0x60000000
BIG = 1 << 40
SIZES = dict(V=3, N=17, T=5, D=20)


def compact(p=(A, B_, C, D_, E), **kw):
    s = {**SIZES, **kw}
    return _lib.load().vivit_embedding_compact_f32(*p, s["V"], s["N"], s["T"], s["D"], None)


def gram(p=(A, B_, C), ws=WS, wsb=BIG, **kw):
    s = {**SIZES, **kw}
    return _lib.load().vivit_embedding_gram_f32(*p, s["V"], s["N"], s["T"], s["D"], 1.0, 0.0, ws, wsb, None)


def need(**kw):
    s = {**SIZES, **kw}
    return _lib.load().vivit_embedding_gram_f32_workspace_bytes(s["V"], s["N"], s["T"], s["D"])


def vmp(p=(A, B_, C, D_, E), F=2, W=7, **kw):
    s = {**SIZES, **kw}
    return _lib.load().vivit_embedding_vmp_f32(*p, F, s["V"], s["N"], s["T"], s["D"], W, None)


def vtmp(p=(A, B_, C, D_), F=2, W=7, **kw):
    s = {**SIZES, **kw}
    return _lib.load().vivit_embedding_vtmp_f32(*p, F, s["V"], s["N"], s["T"], s["D"], W, None)


def mjp(p=(A, B_, C), W=7, **kw):
    s = {**SIZES, **kw}
    return _lib.load().vivit_embedding_weight_mjp_f32(*p, s["V"], s["N"], s["T"], s["D"], W, None)


ENTRIES = {"compact": (compact, 5), "gram": (gram, 3), "vmp": (vmp, 5), "vtmp": (vtmp, 4), "weight_mjp": (mjp, 3)}
NAMES = ("vivit_embedding_compact_f32", "vivit_embedding_gram_f32_workspace_bytes", "vivit_embedding_gram_f32", "vivit_embedding_vmp_f32",
         "vivit_embedding_vtmp_f32", "vivit_embedding_weight_mjp_f32")


def test_symbols_are_exported_and_bound():
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.ABI_VERSION == 1008 and lib.vivit_hip_abi_version() == 1008   # exports were only added


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_pointers_are_refused(entry):
    fn, count = ENTRIES[entry]
    ptrs = (A, B_, C, D_, E)[:count]
    for i in range(count):
        assert fn(p=ptrs[:i] + (None,) + ptrs[i + 1:]) == BADARG


@pytest.mark.parametrize("which", ["V", "N", "T", "D"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_non_positive_sizes_are_refused(entry, which):
    fn = ENTRIES[entry][0]
    assert fn(**{which: 0}) == BADARG
    assert fn(**{which: -3}) == BADARG
    assert need(**{which: 0}) == 0 and need(**{which: -3}) == 0


@pytest.mark.parametrize("entry", ["vmp", "vtmp", "weight_mjp"])
def test_non_positive_vocabulary_and_free_axis_are_refused(entry):
    fn = ENTRIES[entry][0]
    assert fn(W=0) == BADARG and fn(W=-1) == BADARG
    if entry != "weight_mjp":
        assert fn(F=0) == BADARG and fn(F=-2) == BADARG


@pytest.mark.parametrize("entry", ENTRIES)
def test_sizes_beyond_the_index_arithmetic_are_unsupported(entry):
    fn = ENTRIES[entry][0]
    assert fn(V=1 << 31) == UNSUPPORTED
    assert fn(N=1 << 31) == UNSUPPORTED
    assert fn(T=1 << 31) == UNSUPPORTED
    assert fn(D=1 << 31) == UNSUPPORTED
    assert fn(N=1 << 16, T=1 << 15) == UNSUPPORTED                  # n T + u leaves 32 bits
    assert fn(V=1 << 20, N=1 << 10, T=1 << 10, D=1 << 30) == UNSUPPORTED
    assert fn(V=1 << 10, N=1 << 10, T=1 << 10, D=1 << 10) == UNSUPPORTED   # 2^40 elements: the one-thread-per-element grid


def test_gram_limits_are_refused_before_the_workspace_check():
    assert gram(N=16 * 65535 + 1, T=1) == UNSUPPORTED               # pairs of sample blocks beyond the grid
    assert gram(V=1021) == UNSUPPORTED                               # class chunk pairs beyond the grid's second dimension
    assert gram(V=1021, ws=None, wsb=0) == UNSUPPORTED
    assert need(V=1021) == 0 and need(N=16 * 65535 + 1, T=1) == 0
    assert gram(V=1020, N=1, T=1, D=1, wsb=16) == WORKSPACE          # (V = 1020 itself is supported)
    assert vmp(F=65536) == UNSUPPORTED
    assert vtmp(F=1 << 31) == UNSUPPORTED
    assert vmp(W=1 << 31) == UNSUPPORTED and vtmp(W=1 << 32) == UNSUPPORTED and mjp(W=1 << 32) == UNSUPPORTED
    assert mjp(W=1 << 30, D=1 << 20, V=1 << 6, N=1 << 5) == UNSUPPORTED   # V N W D elements beyond 2^60


def test_workspace_has_no_vocabulary_or_quadratic_term():
    """The token tables of the sample blocks: 4 (2 N T + N + 17 * 16 ceil(N / 16) T) bytes and four 256-byte alignments, whatever V, D."""
    for V, N, T, D in ((1, 1, 1, 1), (3, 17, 5, 20), (10, 64, 128, 256), (3, 8, 8, 64), (2, 33, 1000, 7)):
        exact = 4 * (2 * N * T + N + 17 * 16 * ((N + 15) // 16) * T)
        assert exact <= need(V=V, N=N, T=T, D=D) <= exact + 4 * 256
    sizes = [need(T=T) for T in (1, 5, 16, 17, 33, 1024)]
    assert sizes[0] > 0 and all(b > a for a, b in zip(sizes, sizes[1:])), sizes


@pytest.mark.parametrize("shape", [(3, 17, 5, 20), (1, 1, 1, 1), (10, 64, 128, 256), (3, 33, 17, 67)])
def test_short_workspace_is_refused(shape):
    kw = dict(zip("VNTD", shape))
    want = need(**kw)
    assert want > 0
    assert gram(wsb=want - 1, **kw) == WORKSPACE
    assert gram(ws=None, wsb=want, **kw) == WORKSPACE
    assert gram(ws=None, wsb=0, **kw) == WORKSPACE
