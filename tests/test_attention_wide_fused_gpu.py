"""``kernels.attention_wide_forward`` and ``kernels.attention_wide_backward`` (csrc/attention_wide_forward.hip,
csrc/attention_wide_backward.hip: head dimensions 129 to 256) against fp64 under the derived bounds of tests/attention_forward_refs.py
and tests/attention_scoremod_refs.py, both generic in ``d`` -- the backward pass on the device's own ``out`` and ``lse`` against the
rule with one factor row, as tests/test_attention_backward_gpu.py checks the narrow kernels -- and what the kernels promise: the same
bytes from a second call, per padded sample the bytes of the sample cut to its length and run alone, NaN and inf at dead positions
of every operand change no byte, dead rows are ``+0``; the module with ``fused_forward=True`` reaches the pair and allocates no
``T x T`` tensor.

On the commit before the feature every test of this file fails: the launchers do not exist and the module allocates ``T x T``."""
import pytest
import torch

import attention_forward_refs as fr
import attention_scoremod_refs as sr
from vivit_amd import _lib, kernels
from vivit_amd.backend import ScaledDotProductAttention

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = dict(causal=True, lengths=(97, 40, 0), window=40, cap=1.5, table="normal")
# (T, d, H, Hkv, N, modifiers).  d: one column into the second half without vector loads (129) and with them (132), a half-full
# second half (192), a ragged edge (255), the full width (256); T: a single row, within a block, three and four key blocks (the
# rescaling and the block range); R = H / Hkv in {1, 2, 4}; every modifier alone and all together
CASES = [(1, 129, 1, 1, 1, {}),
         (17, 132, 2, 1, 2, dict(causal=True)),
         (65, 192, 4, 1, 3, dict(lengths=(65, 17, 0))),
         (65, 255, 2, 2, 1, dict(window=2)),
         (97, 256, 2, 1, 1, dict(window=40)),
         (65, 129, 2, 2, 1, dict(cap=1.5)),
         (17, 192, 2, 1, 2, dict(table="normal")),
         (97, 255, 4, 4, 1, dict(causal=True, window=2, cap=1.5)),
         (97, 256, 4, 2, 3, ALL)]
IDS = [f"T{c[0]}-d{c[1]}-{'-'.join(c[5]) or 'plain'}" for c in CASES]
_OPERANDS = {}


def operands(case):
    """(dout, qkv, scale, table) of a case, seeded, on the CPU; made once and never written to."""
    if case not in _OPERANDS:
        T, d, H, Hkv, N, mods = CASES[case]
        table = sr.make_table(mods.get("table"), 7 * T + d, H, T)
        M, qkv, _, scale = sr.make_case(1000 * T + d, 1, N, T, H, Hkv, d, None, mods.get("causal", False), mods.get("lengths"),
                                        mods.get("window"), mods.get("cap"), table)
        _OPERANDS[case] = (M[0], qkv, scale, table)
    return _OPERANDS[case]


def mod_args(case):
    """The modifiers of a case in the order the refs take them: (causal, lengths, window, cap)."""
    mods = CASES[case][5]
    return mods.get("causal", False), mods.get("lengths"), mods.get("window"), mods.get("cap")


def run(case, dout, qkv, table, lengths="case", saved=None):
    """(out, lse, dqkv) on the device; ``saved``: the (out, lse) the backward pass is given instead of the forward's own."""
    _, _, H, Hkv, _, _ = CASES[case]
    causal, case_lengths, window, cap = mod_args(case)
    kw = dict(num_kv_heads=Hkv, lengths=case_lengths if lengths == "case" else lengths, window=window, softcap=cap,
              bias=None if table is None else table.to(DEV))
    scale = operands(case)[2]
    out, lse = kernels.attention_wide_forward(qkv.to(DEV), H, scale, causal, return_lse=True, **kw)
    o, s = (out, lse) if saved is None else saved
    return out, lse, kernels.attention_wide_backward(dout.to(DEV), qkv.to(DEV), o, s, H, scale, causal, **kw)


def check(name, got, ref, bound):
    """Finite, within the bound, exact zeros at the dead rows (whose bound is 2^-126)."""
    got = got.cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    print(f"{name}: max error / bound = {((got.double() - ref).abs() / bound).max().item():.3g}")
    ok, msg = fr.within(got, ref, bound)
    assert ok, (name, msg)
    assert bool((got[bound == fr.FLT_MIN] == 0).all())


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_cases_against_fp64(case):
    _, _, H, Hkv, _, _ = CASES[case]
    dout, qkv, scale, table = operands(case)
    out, lse, dqkv = run(case, dout, qkv, table)
    ref_out, e_out, ref_lse, e_lse = fr.self_forward(qkv, H, Hkv, scale, *mod_args(case), table)
    check("out", out, ref_out, e_out)
    check("lse", lse, ref_lse, e_lse)
    check("dqkv", dqkv, *(r[0] for r in sr.rule(dout[None], qkv, out.cpu(), H, Hkv, scale, *mod_args(case), table)))


@pytest.mark.parametrize("case", [2, 8], ids=[IDS[2], IDS[8]])
def test_equal_bytes_padded_samples_alone_and_poisoned_dead_positions(case):
    T, _, _, _, N, mods = CASES[case]
    dout, qkv, _, table = operands(case)
    got = run(case, dout, qkv, table)
    assert all(torch.equal(a, b) for a, b in zip(run(case, dout, qkv, table), got))
    for n, L in enumerate(mods["lengths"]):
        if L > 0:   # the sample cut to its length, every operand, with the table's middle slice
            middle = None if table is None else table[:, T - L:T + L - 1].contiguous()
            alone = run(case, dout[n:n + 1, :L], qkv[n:n + 1, :L], middle, lengths=None)
            for name, a, g in zip(("out", "lse", "dqkv"), alone, (got[0][n, :L], got[1][n, :, :L], got[2][n, :L])):
                assert torch.equal(a[0], g), (name, n, L)
    dead = sr.dead(T, mods["lengths"], N)
    d2, q2, o2, l2 = dout.clone(), qkv.clone(), got[0].cpu(), got[1].cpu().transpose(1, 2).contiguous()
    for t in (d2, q2, o2, l2):
        t[dead] = float("nan")
        t[..., ::2][dead] = float("inf")
    poisoned = run(case, d2, q2, table, saved=(o2.to(DEV), l2.transpose(1, 2).contiguous().to(DEV)))
    assert all(torch.equal(a, b) for a, b in zip(poisoned, got))
    for t in (got[0], got[1].transpose(1, 2), got[2]):
        assert bool((t.cpu()[dead] == 0).all()) and not bool(torch.signbit(t.cpu()[dead]).any())


def test_the_launchers_refuse_d_128():
    qkv = torch.zeros(1, 4, 3 * 128, device=DEV)
    with pytest.raises(_lib.VivitHipError, match="vivit_attention_wide_forward_f32"):
        kernels.attention_wide_forward(qkv, 1, 1.0, False)
    with pytest.raises(_lib.VivitHipError, match="vivit_attention_wide_backward_f32"):
        kernels.attention_wide_backward(qkv[..., :128], qkv, qkv[..., :128], qkv[:, :, 0][:, None], 1, 1.0, False)


def test_the_module_reaches_the_pair():
    """GQA, causal, lengths, a cap, d = 192: ``x.grad`` of the module has the bytes of the launcher pair on the same operands."""
    T, d, H, Hkv, lengths = 70, 192, 4, 2, (70, 33, 0)
    g = sr.gen(3)
    x, W = torch.randn(3, T, (H + 2 * Hkv) * d, generator=g).to(DEV).requires_grad_(), torch.randn(3, T, H * d, generator=g).to(DEV)
    module = ScaledDotProductAttention(H, causal=True, num_kv_heads=Hkv, softcap=2.0, fused_forward=True)
    module.set_lengths(lengths)
    (module(x) * W).sum().backward()
    kw = dict(num_kv_heads=Hkv, lengths=lengths, softcap=2.0)
    out, lse = kernels.attention_wide_forward(x.detach(), H, d ** -0.5, True, return_lse=True, **kw)
    ref = kernels.attention_wide_backward(W, x.detach(), out, lse, H, d ** -0.5, True, **kw)
    assert float(ref.abs().max()) > 0 and torch.equal(x.grad, ref)


def test_no_t_by_t_allocation_in_forward_and_backward():
    """N = 1, H = 2, d = 256, T = 1024: one [N, H, T, T] fp32 tensor is 8 MiB; the results (out and x.grad) are 8 MiB together."""
    H, d, T = 2, 256, 1024
    one, results = H * T * T * 4, 4 * T * H * d * 4
    qkv = torch.randn(1, T, 3 * H * d, device=DEV)
    peaks = {}
    for fused in (True, False):
        x = qkv.clone().requires_grad_()
        module = ScaledDotProductAttention(H, causal=True, fused_forward=fused)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        module(x).sum().backward()
        torch.cuda.synchronize()
        peaks[fused] = torch.cuda.max_memory_allocated() - before - results
        assert x.grad is not None and bool(torch.isfinite(x.grad).all())
    print(f"peak beyond the results: fused {peaks[True] / 2**20:.1f} MiB, torch formula {peaks[False] / 2**20:.1f} MiB")
    assert peaks[True] < one, peaks
    assert peaks[False] > one, peaks   # the control
