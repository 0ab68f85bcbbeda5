"""A Gemma-2-style attention leaf -- grouped queries, head dimension 256, causal, a sliding window, a logit cap, a padded batch --
through the factor provider's ``_jac_t_mat_prod`` on the device: it reaches ``kernels.attention_wide_jac_t`` (neither the torch
formula nor the generic rule may be called) and agrees with the fp64 rule within its derived bounds.

On the commit before the feature this fails: a head dimension above 128 went to the torch formula."""
import pytest
import torch

import attention_scoremod_refs as sr
from vivit_amd.backend import ScaledDotProductAttention, extensions

pytestmark = pytest.mark.gpu


def test_a_gemma2_leaf_of_head_dimension_256_runs_on_the_wide_kernels(monkeypatch):
    V, N, T, H, Hkv, d, window, cap = 3, 3, 40, 4, 2, 256, 33, 50.0
    lengths = (40, 17, 0)

    def forbidden(*args, **kwargs):
        raise AssertionError("a head dimension of 256 must run on the HIP kernels")

    monkeypatch.setattr(extensions, "_attention_jac_t_torch", forbidden)
    monkeypatch.setattr(extensions, "_generic_jac_t_mat_prod", forbidden)
    module = ScaledDotProductAttention(H, causal=True, num_kv_heads=Hkv, window=window, softcap=cap)
    scale = module.scale_for(d)
    M, qkv, out, scale = sr.make_case(31, V, N, T, H, Hkv, d, scale, True, lengths, window, cap, None)
    module.set_lengths(list(lengths))
    x = qkv.to("cuda:0")
    module.output = module(x)   # (the forward pass of the engine: it leaves the output and the lengths it used on the leaf)
    G = extensions._jac_t_mat_prod(module, M.to("cuda:0"), x).cpu()
    ref, bound = sr.rule(M, qkv, out, H, Hkv, scale, True, lengths, window, cap, None)
    assert tuple(G.shape) == (V, N, T, (H + 2 * Hkv) * d)
    ok, msg = sr.within(G, ref, bound)
    assert ok, msg
    assert bool((G[:, sr.dead(T, lengths, N)] == 0).all())
