"""Host checks of tests/attention_refs.py (no GPU).  A plain fp32 restatement of the rule in torch stays well inside the derived
bounds on every case of the GPU list, which makes the bounds a property of the reference and of fp32 arithmetic and not of the
kernel they judge; and five named wrong results, the mistakes the chunked, blocked and tiled paths of csrc/attention.hip could
make, each fall outside the bounds on a listed case, so the list can see them."""
import pytest
import torch

import attention_refs as ar

_REFS = {}


def operands(case):
    """The operands of a case as tests/test_attention_rule_gpu.py makes them, with the fp64 reference (computed once)."""
    if case not in _REFS:
        T, d, H, V, N, causal, scale = case
        M, qkv, out, scale = ar.make_case(1000 * T + d, V, N, T, H, d, scale, causal)
        _REFS[case] = (M, qkv, out, scale) + ar.rule(M, qkv, out, H, scale, causal)
    return _REFS[case]


def emulate(M, qkv, out, H, scale, causal, wrong=None):
    """The formula of include/vivit_hip.h in fp32 torch on the CPU.  ``wrong`` names one deliberate mistake:
    ``chunk``        the factor rows of the second chunk are computed from the first chunk's dO
    ``key-block``    the last key block is left out of dQ
    ``query-block``  the last query block is left out of dK and dV
    ``columns``      the head columns >= 16 floor((d - 1) / 16) are left out of S
    ``strict``       the causal test is j < i (a row without a key gives zeros, as the kernel's would)"""
    V, N, T, E = M.shape
    d = E // H
    q, k, v = qkv.view(N, T, 3, H, d).permute(2, 0, 3, 1, 4)
    dO = M.view(V, N, T, H, d).permute(0, 1, 3, 2, 4)
    O = out.view(N, T, H, d).permute(0, 2, 1, 3)
    if wrong == "chunk":
        VC = ar.chunk(d)
        dO = dO.clone()
        dO[VC:2 * VC] = dO[:max(min(VC, V - VC), 0)]
    mask = torch.zeros(T, T, dtype=torch.bool)
    if causal:
        mask = torch.ones(T, T, dtype=torch.bool).triu(0 if wrong == "strict" else 1)
    c = 16 * ((d - 1) // 16) if wrong == "columns" else d
    S = ((q[..., :c] @ k[..., :c].transpose(-1, -2)) * scale).masked_fill(mask, float("-inf"))
    P = torch.exp(S - torch.logsumexp(S, -1, keepdim=True)).masked_fill(mask, 0.0)
    P = torch.where(mask.all(-1, keepdim=True), torch.zeros_like(P), P)
    D = (dO * O).sum(-1, keepdim=True)
    dS = P * (dO @ v.transpose(-1, -2) - D)
    last = ar.BLOCK * ((T - 1) // ar.BLOCK)
    jn = last if wrong == "key-block" else T
    qn = last if wrong == "query-block" else T
    dQ = (dS[..., :jn] @ k[..., :jn, :]) * scale
    dK = (dS[..., :qn, :].transpose(-1, -2) @ q[..., :qn, :]) * scale
    dV = P[..., :qn, :].transpose(-1, -2) @ dO[..., :qn, :]
    return torch.stack((dQ, dK, dV), 0).permute(1, 2, 4, 0, 3, 5).reshape(V, N, T, 3 * E)


def outside(got, ref, bound):
    return not bool(torch.isfinite(got).all()) or not ar.within(got, ref, bound)[0]


@pytest.mark.parametrize("case", ar.CASES, ids=str)
def test_fp32_restatement_stays_within_the_bounds(case):
    T, d, H, V, N, causal, _ = case
    M, qkv, out, scale, ref, bound = operands(case)
    assert ref.shape == bound.shape == (V, N, T, 3 * H * d) and bool((bound > 0).all())
    got = emulate(M, qkv, out, H, scale, causal)
    assert bool(torch.isfinite(got).all())
    ratio = ((got.double() - ref).abs() / bound).max().item()
    print(f"max error / bound = {ratio:.3g}")
    assert ratio <= 0.5, ratio


def test_the_rule_of_the_case_list_holds():
    assert len(set(ar.CASES)) == len(ar.CASES)
    for lo, hi in ((1, 16), (17, 32), (33, 64), (65, 128)):
        mine = [c for c in ar.CASES if lo <= c[1] <= hi]
        VC = ar.chunk(lo)
        assert ar.chunk(hi) == VC
        assert {lo, hi} <= {c[1] for c in mine}, (lo, hi)
        chunks = {(c[3] // VC, c[3] % VC > 0) for c in mine}
        assert {(0, True), (1, True), (2, True)} <= chunks and {(1, False), (2, False)} & chunks, (lo, hi, chunks)
        assert {32, 64} & {c[0] for c in mine} and {33, ar.TB} & {c[0] for c in mine}, (lo, hi)
        assert {False, True} == {c[5] for c in mine}
    assert {1, 5, 16, 17, 32, 33, 64, ar.TB} <= {c[0] for c in ar.CASES}
    assert any(c[6] is not None and c[6] < 0 for c in ar.CASES) and any(c[6] == 0.0 for c in ar.CASES)


def test_zero_scale_reference():
    case = next(c for c in ar.CASES if c[6] == 0.0)
    T, d, H, V, N, causal, _ = case
    _, _, _, scale, ref, bound = operands(case)
    E = H * d
    assert scale == 0.0 and bool((ref[..., :2 * E] == 0).all()) and bool((bound[..., :2 * E] == ar.FLT_MIN).all())
    assert float(ref[..., 2 * E:].abs().max()) > 0


@pytest.mark.parametrize("wrong", ["chunk", "key-block", "query-block", "columns", "strict"])
def test_named_wrong_result_falls_outside_the_bounds(wrong):
    caught = []
    for case in ar.CASES:
        T, d, H, V, N, causal, _ = case
        M, qkv, out, scale, ref, bound = operands(case)
        if outside(emulate(M, qkv, out, H, scale, causal, wrong), ref, bound):
            caught.append(case)
    print(f"{wrong}: seen by {len(caught)} of {len(ar.CASES)} cases")
    assert caught
    # seen where the path is new, not only by an old case: a second chunk exists, more than one block, a cut tile column
    if wrong == "chunk":
        assert all(c[3] > ar.chunk(c[1]) for c in caught)
        for lo, hi in ((1, 16), (17, 32), (33, 64), (65, 128)):
            assert any(lo <= c[1] <= hi for c in caught), (lo, hi)
    if wrong in ("key-block", "query-block"):
        assert any(c[0] in (32, 64) for c in caught) and any(c[0] in (33, ar.TB) for c in caught)
    if wrong == "columns":
        assert any(c[1] in (33, 65) for c in caught) and any(c[1] in (17, 127) for c in caught)
    if wrong == "strict":
        assert all(c[5] for c in caught)
