"""Host checks of tests/embedding_refs.py (no GPU).  A plain fp32 restatement of the Embedding rule's operations in torch stays
well inside the derived bounds on every case of the GPU lists, which makes the bounds a property of the reference and of fp32
arithmetic and not of the kernels they judge; four named wrong Gram matrices, the mistakes the chunked and joined paths of
csrc/embedding.hip could make, each fall outside the bound on a listed case; the staircase constructions have the token tables
and shared ranks the lists claim; and the slots torch computes for the kernels are those of the reference."""
import pytest
import torch

import embedding_refs as er
from vivit_amd import kernels

ALL = [("edge",) + c for c in er.CASES] + [("staircase",) + c for c in er.STAIRCASE_CASES] + [("large", False), ("large", True)]
_CASES = {}


def case_of(key):
    if key not in _CASES:
        make = {"edge": er.case_of, "staircase": er.staircase_of, "large": er.large_id_case}[key[0]]
        _CASES[key] = make(*key[1:])
    return _CASES[key]


def name(key):
    return "-".join(str(k) for k in key)


# ---- the operations in fp32 --------------------------------------------------------------------------------------------------
def compact32(case, padding=True):
    """(B [V, N, T, D] fp32, ids [N, T]): the rows of a slot added in ascending t.  ``padding=False``: the padding token is a token."""
    V, N, T, D = case.M.shape
    ids, _, _, _, slot = kernels.embedding_token_slots(case.idx, case.padding_idx if padding else None)
    dest = (slot + (T + 1) * torch.arange(N).unsqueeze(1)).reshape(-1)
    B = torch.zeros(V, N * (T + 1), D).index_add_(1, dest, case.M.reshape(V, N * T, D))
    return B.view(V, N, T + 1, D)[:, :, :T].contiguous(), ids.long()


def factor32(case, B, ids):
    """The rows of B at their (renumbered) tokens: [V, N, Wr, D] fp32."""
    V, N, T, D = B.shape
    Wr = case.tokens.numel()
    col = torch.searchsorted(case.tokens, ids.clamp_min(0))
    dest = torch.where(ids >= 0, col + (Wr + 1) * torch.arange(N).unsqueeze(1), torch.full_like(ids, Wr)).reshape(-1)   # -1 slots: a spare row
    Vt = torch.zeros(V, N * (Wr + 1), D).index_add_(1, dest, B.reshape(V, N * T, D))
    return Vt.view(V, N, Wr + 1, D)[:, :, :Wr]


def gram32(case, wrong=None):
    """``wrong`` names one deliberate mistake of the Gram matrix:
    ``rank``     the tokens of rank >= 256 in the row sample block's table are left out of the join
    ``chunk``    the column classes of every class chunk are read from chunk 0
    ``columns``  the columns >= 64 are left out
    ``minus``    the tokens of -1 slots are treated as a common token: -1 slots stand for the padding positions, so the padding
                 rows are added up and joined like any token's (without padding a -1 slot holds no row and nothing can change)"""
    V, N = case.V, case.N
    Vt = factor32(case, *compact32(case, padding=wrong != "minus"))
    if wrong == "columns":
        Vt = Vt[..., :64]
    if wrong == "rank":
        G = torch.zeros(V, N, V, N)
        for bi, tab in enumerate(case.block_tables()):
            keep = torch.isin(case.tokens, tab[:er.JOIN_PASS])
            ri = slice(er.SAMPLE_BLOCK * bi, er.SAMPLE_BLOCK * (bi + 1))
            rows = Vt[:, ri][:, :, keep]
            for bj in range(bi + 1):
                rj = slice(er.SAMPLE_BLOCK * bj, er.SAMPLE_BLOCK * (bj + 1))
                cols = Vt[:, rj][:, :, keep]
                blk = torch.einsum("vnwd,umwd->vnum", rows, cols)
                G[:, ri, :, rj] = blk
                G[:, rj, :, ri] = blk.permute(2, 3, 0, 1)
        return G.reshape(V * N, V * N)
    A = Vt.reshape(V * N, -1)
    G = A @ A.T
    if wrong == "chunk":
        G = G.view(V, N, V, N)[:, :, torch.arange(V) % er.CLASS_CHUNK].reshape(V * N, V * N)
    return G


def ratio(got, ref, bound):
    err = (got.double() - ref).abs()
    assert bool(torch.isfinite(got).all()) and bool((err[bound == 0] == 0).all())
    return (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0


@pytest.mark.parametrize("key", ALL, ids=name)
def test_fp32_restatement_stays_within_the_bounds(key):
    case = case_of(key)
    B, ids = compact32(case)
    assert torch.equal(ids, case.ids())
    r = {"compact": ratio(B, *case.compact()), "gram": ratio(gram32(case), *case.gram())}
    if key[0] != "large":                                              # (an axis of length W beyond here)
        V, N, D, W = case.V, case.N, case.D, case.W
        Vt = factor32(case, B, ids)
        g = er.gen(7)
        mat = torch.randn(2, V, N, generator=g)
        ref, bound = case.vmp(mat)
        r["vmp"] = ratio(torch.einsum("fvn,vnwd->fwd", mat, Vt), ref[:, case.tokens], bound[:, case.tokens])
        mat = torch.randn(2, W, D, generator=g)
        r["vtmp"] = ratio(torch.einsum("fwd,vnwd->fvn", mat[:, case.tokens], Vt), *case.vtmp(mat))
        ref, bound = case.factor()
        r["weight_mjp"] = ratio(Vt, ref[:, :, case.tokens], bound[:, :, case.tokens])
    print(", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    # a sum of m rows takes m - 1 roundings and its bound counts m (tests/embedding_refs.py): up to (m - 1) / m of it, m <= T, is
    # what correct fp32 arithmetic can reach in the copies; everything else has to stay below half of its bound
    copies = ("compact", "weight_mjp")
    assert all(v <= (case.T - 1) / case.T for k, v in r.items() if k in copies), r
    assert all(v <= 0.5 for k, v in r.items() if k not in copies), r


@pytest.mark.parametrize("wrong", ["rank", "chunk", "columns", "minus"])
def test_named_wrong_gram_falls_outside_the_bound(wrong):
    caught = []
    for key in ALL:
        case = case_of(key)
        if not er.within(gram32(case, wrong), *case.gram())[0]:
            caught.append(key)
    print(f"{wrong}: seen by {len(caught)} of {len(ALL)} cases")
    assert caught
    if wrong == "rank":       # every construction with a table beyond one pass, under both numbers of class chunks
        assert {k[1:4] for k in caught} == {c for c, w in er.STAIRCASE.items() if w["table"] > er.JOIN_PASS}
        assert {k[4] for k in caught} == {5, 9}
    if wrong == "chunk":
        assert all(case_of(k).V > er.CLASS_CHUNK for k in caught) and {case_of(k).V for k in caught} >= {5, 8, 9}
    if wrong == "columns":
        assert {case_of(k).D for k in caught} == {67, 128, 129}
    if wrong == "minus":
        assert all(case_of(k).padding_idx is not None for k in caught) and ("large", True) in caught


@pytest.mark.parametrize("geometry", list(er.STAIRCASE), ids=str)
def test_staircase_geometry(geometry):
    N, T, S = geometry
    for V, D in ((5, 4), (9, 20)):
        case = case_of(("staircase", N, T, S, V, D))
        er.check_staircase(case, N, T, S)
        assert case.W == S * (N - 1) + T == int(case.idx.max()) + 1 and int(case.idx.min()) == 0
        assert torch.equal(case.idx.sort(1).values, S * torch.arange(N).unsqueeze(1) + torch.arange(T))
        tabs = case.block_tables()
        assert all(torch.equal(t, 16 * S * b + torch.arange(t.numel())) for b, t in enumerate(tabs))
        shared = case.shared_tokens()
        assert bool((shared.diagonal(1) == T - S).all()) and bool((shared.diagonal(2) == max(T - 2 * S, 0)).all())


@pytest.mark.parametrize("key", ALL, ids=name)
def test_token_slots_are_those_of_the_reference(key):
    case = case_of(key)
    ids, perm, start, cnt, slot = kernels.embedding_token_slots(case.idx, case.padding_idx)
    assert ids.dtype == torch.int32 and torch.equal(ids.long(), case.ids())
    valid = torch.ones_like(case.idx, dtype=torch.bool) if case.padding_idx is None else case.idx != case.padding_idx
    assert torch.equal(cnt.long().sum(1), valid.sum(1)) and bool((slot[~valid] == case.T).all())
    assert torch.equal(ids.long().gather(1, slot.clamp_max(case.T - 1))[valid], case.idx[valid])


def test_large_ids_reach_the_top_of_int32():
    for pad in (False, True):
        case = case_of(("large", pad))
        ids = case.ids()
        assert int(ids.max()) == 2 ** 31 - 2 and case.W == 2 ** 31 - 1
        assert int((ids >= 0).sum()) == 2 * case.T - (1 if pad else 0)
        assert int(case.shared_tokens()[0, 1]) == 2
        # the unsigned order the kernels search in: tokens ascending, -1 behind the largest of them
        u = ids.to(torch.int32).view(torch.uint8).view(case.N, case.T, 4).long()
        key = u[..., 0] + (u[..., 1] << 8) + (u[..., 2] << 16) + (u[..., 3] << 24)
        assert bool((key[:, 1:] >= key[:, :-1]).all())
