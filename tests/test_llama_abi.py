"""The entry points of csrc/llama_rules.hip (include/vivit_hip.h): their refusing half.

No GPU is needed and none is used: every call below must be answered by the host-side checks before anything is enqueued (as
tests/test_seq_linear_abi.py does; the pointers are fake non-null addresses that the host never dereferences)."""
import pytest

from vivit_amd import _lib

OK, BADARG, WORKSPACE, LAUNCH, UNSUPPORTED = 0, -1, -2, -3, -4
P = 0x7F0000001000  # fake device pointers
A, B_, C, D_, E_, F_ = (P + i * 0x10000000 for i in range(6))
BIG = (1 << 31, 1 << 62)

# name -> (number of pointers, default sizes in call order, trailing non-size arguments before the stream)
ENTRIES = {
    "vivit_rms_norm_stats_f32": (2, dict(rows=3, L=8), (1e-5,)),
    "vivit_rms_norm_rules_f32": (6, dict(V=2, rows=3, L=8), ()),
    "vivit_rms_norm_position_sums_f32": (4, dict(V=2, N=3, A=4, D=8), ()),
    "vivit_gate_jac_t_f32": (5, dict(V=2, n=8), ()),
    "vivit_rope_jac_t_f32": (4, dict(R=2, T=3, H=2, d=4), ()),
}
ARGC = {"vivit_rms_norm_stats_f32": 6, "vivit_rms_norm_rules_f32": 10, "vivit_rms_norm_position_sums_f32": 9, "vivit_gate_jac_t_f32": 8,
        "vivit_rope_jac_t_f32": 9}
CASES = [(name, which) for name, (_, sizes, _) in ENTRIES.items() for which in sizes]


def call(name, ptrs=None, **kw):
    nptr, sizes, tail = ENTRIES[name]
    ptrs = (A, B_, C, D_, E_, F_)[:nptr] if ptrs is None else ptrs
    s = {**sizes, **kw}
    return getattr(_lib.load(), name)(*ptrs, *s.values(), *tail, None)


def nulls(name):
    return (None,) * ENTRIES[name][0]


@pytest.mark.parametrize("name", list(ENTRIES))
def test_symbols_are_exported_and_bound(name):
    lib = _lib.load()
    assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1] and len(_lib.SIGNATURES[name][1]) == ARGC[name]
    assert _lib.ABI_VERSION == 1008 and lib.vivit_hip_abi_version() == 1008   # exports were only added


@pytest.mark.parametrize("name,which", CASES)
def test_any_zero_size_launches_nothing(name, which):
    assert call(name, **{which: 0}) == OK
    assert call(name, **{which: 0}, ptrs=nulls(name)) == OK                   # and reads no pointer


@pytest.mark.parametrize("name,which", CASES)
def test_negative_sizes_are_refused(name, which):
    assert call(name, **{which: -1}) == BADARG
    assert call(name, **{which: -(1 << 40)}) == BADARG
    assert call(name, **{which: -1}, ptrs=nulls(name)) == BADARG


@pytest.mark.parametrize("name,which", CASES)
def test_sizes_beyond_the_index_arithmetic_are_unsupported(name, which):
    for big in BIG:
        if name == "vivit_rope_jac_t_f32" and which == "d":
            assert call(name, d=big) == UNSUPPORTED and call(name, d=big + 1) == BADARG   # (odd comes first)
        else:
            assert call(name, **{which: big}) == UNSUPPORTED


def test_products_of_sizes_beyond_the_grid_are_unsupported():
    assert call("vivit_rms_norm_rules_f32", V=1 << 16, rows=1 << 15) == UNSUPPORTED              # V rows leaves 31 bits
    assert call("vivit_rms_norm_position_sums_f32", V=1 << 16, N=1 << 15) == UNSUPPORTED
    assert call("vivit_rms_norm_position_sums_f32", V=1 << 12, N=1 << 12, D=1 << 15) == UNSUPPORTED   # V N ceil(D / 256) blocks
    assert call("vivit_rope_jac_t_f32", R=1 << 16, T=1 << 15) == UNSUPPORTED                     # R T rows
    assert call("vivit_rope_jac_t_f32", H=1 << 15, d=1 << 15) == UNSUPPORTED                     # 3 H d, the length of a row
    assert call("vivit_rope_jac_t_f32", T=1 << 16, d=1 << 15) == UNSUPPORTED                     # T d, twice the tables


def test_null_pointers_are_refused():
    full = (A, B_, C, D_, E_, F_)
    for name, (nptr, _, _) in ENTRIES.items():
        optional = {"vivit_rms_norm_rules_f32": {2, 4, 5}, "vivit_gate_jac_t_f32": {1, 2, 3, 4}}.get(name, set())
        for which in range(nptr):
            if which not in optional:
                assert call(name, ptrs=full[:which] + (None,) + full[which + 1:nptr]) == BADARG, (name, which)
    # RMSNorm rules: gamma may be null, out or w may be null, not both
    assert call("vivit_rms_norm_rules_f32", ptrs=(A, B_, C, D_, None, None)) == BADARG
    # gate: either output may be null with its operand (a belongs to Gb, b to Ga), not both outputs; an output without its operand is refused
    assert call("vivit_gate_jac_t_f32", ptrs=(A, B_, C, None, None)) == BADARG
    assert call("vivit_gate_jac_t_f32", ptrs=(A, B_, None, D_, None)) == BADARG     # Ga wants b
    assert call("vivit_gate_jac_t_f32", ptrs=(A, None, C, None, E_)) == BADARG      # Gb wants a
    assert call("vivit_gate_jac_t_f32", ptrs=(A, None, None, None, None)) == BADARG


def test_rotary_head_dimension_must_be_even():
    for d in (1, 3, 129):
        assert call("vivit_rope_jac_t_f32", d=d) == BADARG
        assert call("vivit_rope_jac_t_f32", d=d, ptrs=nulls("vivit_rope_jac_t_f32")) == BADARG


def test_a_negative_or_nan_eps_is_refused():
    lib = _lib.load()
    assert lib.vivit_rms_norm_stats_f32(A, B_, 3, 8, -1.0, None) == BADARG
    assert lib.vivit_rms_norm_stats_f32(A, B_, 3, 8, float("nan"), None) == BADARG
