"""``kernels.rope_jac_t(..., num_kv_heads=Hkv)`` (csrc/llama_rules.hip, ``vivit_rope_gqa_jac_t_f32``): the rotary rule on the packed
projection of grouped-query attention, ``H + Hkv`` rotated heads and ``Hkv d`` copied columns, against the fp64 reference of
tests/attention_gqa_refs.py under the bound of tests/llama_refs.py -- out of place, in place and with an operand 4 bytes off a 16-byte
boundary, between guard words."""
import pytest
import torch

import attention_gqa_refs as gr
import llama_refs as lr
from vivit_amd import kernels
from vivit_amd.backend import RotaryEmbedding

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = 5   # (r) rows: V N of the caller


def case(H, Hkv, d, T):
    g = gr.gen(d + 10 * T + H + 100 * Hkv)
    return lr.generic(g, ROWS, T, (H + 2 * Hkv) * d), gr.rope_tables(T, d)


@pytest.mark.parametrize("T", gr.ROPE_T)
@pytest.mark.parametrize("d", gr.ROPE_D)
@pytest.mark.parametrize("H,Hkv", gr.ROPE_HEADS)
def test_rope_gqa(H, Hkv, d, T):
    M, (cos, sin) = case(H, Hkv, d, T)
    ref, bound = gr.rope(M, cos, sin, H, Hkv)
    cd, sd = cos.to(DEV), sin.to(DEV)
    v0 = (H + Hkv) * d
    results = {}
    for mode in ("out_of_place", "in_place", "offset4"):
        shift = mode == "offset4"
        if mode == "in_place":
            buf, view = lr.guarded(M.shape, DEV)
            view.copy_(M)
            G = kernels.rope_jac_t(view, cd, sd, H, out=view, num_kv_heads=Hkv)
        else:
            Md = lr.misaligned(M.to(DEV)) if shift else M.to(DEV)
            assert Md.data_ptr() % 16 == (4 if shift else 0)
            buf, view = lr.guarded(M.shape, DEV, shift)
            G = kernels.rope_jac_t(Md, cd, sd, H, out=view, num_kv_heads=Hkv)
            assert torch.equal(Md.cpu(), M)                                    # the input is left alone
        assert G is view and lr.guards_intact(buf, view, shift)
        got = G.cpu()
        assert bool(torch.isfinite(got).all())
        ok, msg = gr.within(got, ref, bound)
        assert ok, f"H={H} Hkv={Hkv} d={d} T={T} {mode}: {msg}"
        assert torch.equal(got[..., v0:], M[..., v0:])                         # the v part: bit for bit
        results[mode] = got
    assert torch.equal(results["in_place"], results["out_of_place"]) and torch.equal(results["offset4"], results["out_of_place"])
    if Hkv == H:                                                               # three equal thirds: the bytes of the old entry point
        assert torch.equal(kernels.rope_jac_t(M.to(DEV), cd, sd, H).cpu(), results["out_of_place"])


@pytest.mark.parametrize("H,Hkv,d,T", [(4, 2, 6, 33), (3, 1, 64, 33), (2, 1, 2, 5)])
def test_rule_inverts_the_forward_pass_of_the_module(H, Hkv, d, T):
    x = lr.generic(gr.gen(d + T), 4, T, (H + 2 * Hkv) * d)
    mod = RotaryEmbedding(H, num_kv_heads=Hkv)
    y = mod(x.to(DEV))
    assert torch.equal(y[..., (H + Hkv) * d:].cpu(), x[..., (H + Hkv) * d:])
    back = kernels.rope_jac_t(y, *mod.tables(T, d, DEV, torch.float32), H, num_kv_heads=Hkv).cpu()
    a = x.double().abs()[..., :(H + Hkv) * d].view(4, T, H + Hkv, 2, d // 2)
    pair = (a[:, :, :, 0] + a[:, :, :, 1]).unsqueeze(3).expand(-1, -1, -1, 2, -1).reshape(4, T, -1)   # 14 eps (|x1| + |x2|): llama_refs
    bound = torch.cat((14 * gr.EPS * pair, torch.zeros(4, T, Hkv * d, dtype=torch.float64)), -1)
    ok, msg = gr.within(back, x.double(), bound)
    assert ok, msg


def test_shape_errors_come_before_any_launch():
    z = lambda *s: torch.zeros(*s, device=DEV)   # noqa: E731
    with pytest.raises(ValueError, match="multiple of num_kv_heads"):
        kernels.rope_jac_t(z(2, 4, 40), z(4, 2), z(4, 2), 4, num_kv_heads=3)
    with pytest.raises(ValueError, match=r"\(4 \+ 2 \* 2\) heads"):
        kernels.rope_jac_t(z(2, 4, 24), z(4, 1), z(4, 1), 4, num_kv_heads=2)      # d = 3 is odd
    with pytest.raises(ValueError, match="cos and sin"):
        kernels.rope_jac_t(z(2, 4, 32), z(3, 2), z(3, 2), 4, num_kv_heads=2)      # tables of T = 3
