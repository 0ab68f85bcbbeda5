"""``kernels.attention_wide_jac_t`` (csrc/attention_wide.hip, ``vivit_attention_wide_jac_t_f32``: head dimensions 129 to 256) against
the fp64 rule under the derived bounds of tests/attention_scoremod_refs.py, which is generic in ``d``, and the promises of the
contract: equal bytes call to call and for a ``(v, n)`` slice run alone, NaN at dead positions reaches nothing and dead rows are
``+0``, no ``T x T`` allocation."""
import pytest
import torch

import attention_scoremod_refs as sr
from vivit_amd import kernels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = dict(causal=True, lengths=(17, 0), window=40, cap=1.5, table="normal")
# (T, d, H, Hkv, V, N, modifiers).  d: one column into the second half without vector loads (129) and with them (132), a half-full
# second half (192), a ragged edge (255), the full width (256); T: 1, within a block, one row and one block plus one row beyond;
# V: zero, one and two full chunks of two rows plus a remainder; R = H / Hkv in {1, 2, 4}; every modifier alone and all together
CASES = [(1, 129, 1, 1, 1, 1, {}),
         (17, 132, 2, 1, 3, 2, dict(causal=True)),
         (65, 192, 4, 1, 5, 2, dict(lengths=(17, 0))),
         (65, 255, 2, 2, 3, 1, dict(window=2)),
         (65, 256, 2, 1, 1, 2, dict(window=40)),
         (33, 129, 2, 2, 3, 1, dict(cap=1.5)),
         (17, 192, 2, 1, 1, 2, dict(table="normal")),
         (33, 255, 4, 4, 5, 2, dict(causal=True, window=2, cap=1.5)),
         (65, 256, 4, 2, 5, 2, ALL)]
_OPERANDS = {}


def operands(case):
    """(M, qkv, out, scale, table) of a case, seeded, on the CPU; made once and never written to."""
    if case not in _OPERANDS:
        T, d, H, Hkv, V, N, mods = CASES[case]
        table = sr.make_table(mods.get("table"), 7 * T + d, H, T)
        _OPERANDS[case] = sr.make_case(1000 * T + d, V, N, T, H, Hkv, d, None, mods.get("causal", False), mods.get("lengths"),
                                       mods.get("window"), mods.get("cap"), table) + (table,)
    return _OPERANDS[case]


def run(M, qkv, out, H, Hkv, scale, mods, table, lengths="case"):
    return kernels.attention_wide_jac_t(M.to(DEV), qkv.to(DEV), out.to(DEV), H, scale, mods.get("causal", False), num_kv_heads=Hkv,
                                        lengths=mods.get("lengths") if lengths == "case" else lengths, window=mods.get("window"),
                                        softcap=mods.get("cap"), bias=None if table is None else table.to(DEV)).cpu()


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda i: f"T{CASES[i][0]}-d{CASES[i][1]}-{'-'.join(CASES[i][6]) or 'plain'}")
def test_cases_against_the_fp64_rule(case):
    T, d, H, Hkv, V, N, mods = CASES[case]
    M, qkv, out, scale, table = operands(case)
    got = run(M, qkv, out, H, Hkv, scale, mods, table)
    ref, bound = sr.rule(M, qkv, out, H, Hkv, scale, mods.get("causal", False), mods.get("lengths"), mods.get("window"), mods.get("cap"), table)
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    print(f"max error / bound = {((got.double() - ref).abs() / bound).max().item():.3g}")
    ok, msg = sr.within(got, ref, bound)
    assert ok, msg


@pytest.mark.parametrize("case", [1, 8])   # (two live samples without lengths; all modifiers with a dead second sample)
def test_equal_bytes_call_to_call_and_for_a_slice_run_alone(case):
    T, d, H, Hkv, V, N, mods = CASES[case]
    M, qkv, out, scale, table = operands(case)
    G = run(M, qkv, out, H, Hkv, scale, mods, table)
    assert torch.equal(G, run(M, qkv, out, H, Hkv, scale, mods, table))
    for v, n in ((0, 0), (1, 1), (V - 2, 1), (V - 1, 0)):   # both places of a chunk and the ragged last chunk, either sample
        lengths = None if mods.get("lengths") is None else mods["lengths"][n:n + 1]
        alone = run(M[v:v + 1, n:n + 1].contiguous(), qkv[n:n + 1].contiguous(), out[n:n + 1].contiguous(), H, Hkv, scale, mods, table,
                    lengths=lengths)
        assert torch.equal(G[v, n], alone[0, 0]), (v, n)


@pytest.mark.parametrize("case", [2, 8])
def test_nan_at_dead_positions_reaches_nothing_and_dead_rows_are_plus_zero(case):
    T, d, H, Hkv, V, N, mods = CASES[case]
    M, qkv, out, scale, table = operands(case)
    dead = sr.dead(T, mods["lengths"], N)
    M2, q2, o2 = M.clone(), qkv.clone(), out.clone()
    M2[:, dead], q2[dead], o2[dead] = float("nan"), float("nan"), float("-inf")
    G = run(M2, q2, o2, H, Hkv, scale, mods, table)
    assert torch.equal(G, run(M, qkv, out, H, Hkv, scale, mods, table))
    assert bool((G[:, dead] == 0).all()) and not bool(torch.signbit(G[:, dead]).any())


@pytest.mark.parametrize("mods", [{}, dict(causal=True, window=40, cap=1.5, table="normal")], ids=["plain", "all"])
def test_no_t_by_t_allocation(mods):
    V, N, T, H, Hkv, d = 2, 1, 256, 2, 1, 256
    g = sr.gen(5)
    M, qkv, out = (torch.randn(s, generator=g).to(DEV) for s in ((V, N, T, H * d), (N, T, (H + 2 * Hkv) * d), (N, T, H * d)))
    table = None if "table" not in mods else sr.make_table("normal", 1, H, T).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    G = kernels.attention_wide_jac_t(M, qkv, out, H, d ** -0.5, mods.get("causal", False), num_kv_heads=Hkv, window=mods.get("window"),
                                     softcap=mods.get("cap"), bias=table)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before - G.numel() * 4
    assert extra < V * N * H * T * T * 4, extra   # below one fp32 [V, N, H, T, T]
