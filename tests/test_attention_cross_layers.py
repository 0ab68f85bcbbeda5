"""Cross-attention (``MultiheadCrossAttention`` / ``ScaledDotProductCrossAttention``) in the factor provider, end to end on a small
encoder-decoder -- host and hip flavours, built as tests/test_attention_masked_layers.py is.  One id tensor ``X [N, Ts + Tt]`` carries
the source and the target tokens; a test-local container slices it, so that the brute-force oracle can differentiate the model of one
input.  Source side: Embedding -> RMSNorm -> MultiheadSelfAttention.  Target side: Embedding -> causal MultiheadSelfAttention ->
MultiheadCrossAttention on (target stream, encoder output) -> Linear head -> Permute -> per-position cross entropy with
``ignore_index``.  Both sides are right-padded; one sample has an empty source, one an empty target.

The factors of the padded batch equal the brute-force oracle's on the fp64 model; their per-sample GGN equals the one of each sample
cut to its two lengths and run ALONE through a model that knows nothing of lengths; the Gram matrix of the ViViT closures is the Gram
matrix of those factors.  Tolerances: those of tests/test_attention_gqa_layers.py for the factors and of
tests/test_loss_positions_layers.py for the Gram matrix, unchanged; ``ggn_close`` as tests/test_attention_masked_layers.py writes it.

On the commit before the feature this file fails at import: the modules do not exist."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import loss_weighted_refs as refs
from helpers import OracleBackend, set_kernel_backend
from oracle import vivit_oracle as oracle
from vivit_amd import kernels
from vivit_amd.backend import (MultiheadCrossAttention, MultiheadSelfAttention, Permute, ScaledDotProductCrossAttention, SqrtGGNExact,
                               ViViTGGNExact, backpack, extend)
from vivit_amd.backend import extensions as ext

FLAVOURS = [pytest.param("host", id="host"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
F64 = torch.float64
PAD = -100
VOCAB, E, H, HKV, C, TS, TT = 7, 8, 4, 2, 3, 4, 5
SRC = (4, 2, 0, 3)              # source lengths: sample 2 has an empty source (its targets see nothing: rows of zeros, not NaN)
TGT = (5, 3, 2, 0)              # target lengths: sample 3 is padding from its first position on
N = len(SRC)


@pytest.fixture(params=FLAVOURS)
def device(request):
    if request.param == "host":
        set_kernel_backend(OracleBackend())
        yield torch.device("cpu")
        set_kernel_backend(None)
    else:
        set_kernel_backend(None)
        yield torch.device("cuda:0")


class EncoderDecoder(nn.Module):
    """The model of the module docstring on ``X [N, ts + Tt]`` (token ids, integer or floating: the brute-force oracle differentiates a
    model of a floating ``X``).  ``layers``: cross-attention layers in a row, every one on the same encoder output."""

    def __init__(self, layers=1):
        super().__init__()
        self.ts = TS
        self.src_embed, self.src_norm = nn.Embedding(VOCAB, E), nn.RMSNorm(E, eps=1e-5)
        self.encoder = MultiheadSelfAttention(E, H, num_kv_heads=HKV)
        self.tgt_embed = nn.Embedding(VOCAB, E)
        self.self_attention = MultiheadSelfAttention(E, H, causal=True, num_kv_heads=HKV)
        self.cross = nn.ModuleList(MultiheadCrossAttention(E, H, num_kv_heads=HKV) for _ in range(layers))
        self.head, self.permute = nn.Linear(E, C), Permute(0, 2, 1)

    def set_lengths(self, src, tgt):
        self.encoder.set_lengths(src)
        self.self_attention.set_lengths(tgt)
        for layer in self.cross:
            layer.set_lengths(tgt, src)

    def frozen_side(self):
        """What produces the keys and values: the encoder and the cross-attention's projection of its output."""
        return [self.src_embed, self.src_norm, self.encoder] + [layer.kv_proj for layer in self.cross]

    def forward(self, X):
        ids = X.long()
        memory = self.encoder(self.src_norm(self.src_embed(ids[:, :self.ts])))
        h = self.self_attention(self.tgt_embed(ids[:, self.ts:]))
        for layer in self.cross:
            h = layer(h, memory)
        return self.permute(self.head(h))


def make_problem(layers=1, frozen=False):
    torch.manual_seed(0)
    model = EncoderDecoder(layers)
    g = torch.Generator().manual_seed(1)
    for m in model.modules():
        if isinstance(m, nn.Linear):
            for p in m.parameters():
                p.data.copy_(torch.rand(p.shape, generator=g) * 1.2 - 0.5)
        if isinstance(m, nn.RMSNorm):
            m.weight.data.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
    X, y = torch.randint(0, VOCAB, (N, TS + TT), generator=g), torch.randint(0, C, (N, TT), generator=g)
    for n, L in enumerate(TGT):
        y[n, L:] = PAD
    if frozen:
        for m in model.frozen_side():
            m.requires_grad_(False)
    return model, X, y, nn.CrossEntropyLoss(ignore_index=PAD, reduction="sum")


_REFERENCE = {}


def reference(layers=1, frozen=False):
    """fp64, computed once per problem and never written to: (a) the oracle's factors of the PADDED batch through the model with
    lengths, one per trainable parameter; (b) per sample with a source and a target the GGN of the sample cut to its two lengths and
    run alone through the model WITHOUT lengths: J^T H J with J and the Hessian H of the summed cross entropy by autograd."""
    key = (layers, frozen)
    if key not in _REFERENCE:
        model, X, y, lossf = make_problem(layers, frozen)
        ref = model.double()
        ref.set_lengths(list(SRC), list(TGT))
        Xf = X.double()
        out = ref(Xf).detach()
        S = refs.exact_factor(out, lossf, y).flatten(2)
        V_ref = oracle.sqrt_ggn_factors(ref, Xf, S, None)
        ref.set_lengths(None, None)
        ggn = []
        for n, (Ls, Lt) in enumerate(zip(SRC, TGT)):
            if Ls == 0 or Lt == 0:   # (no sequence of no tokens can be run alone)
                ggn.append(None)
                continue
            ref.ts = Ls
            alone = torch.cat((Xf[n:n + 1, :Ls], Xf[n:n + 1, TS:TS + Lt]), 1)
            jac = oracle.per_sample_jacobians(ref, alone)                               # [1, C Lt, *param]
            J = torch.cat([j.reshape(C * Lt, -1) for j in jac], 1)
            z = ref(alone).detach()
            Hz = torch.autograd.functional.hessian(lambda o: F.cross_entropy(o, y[n:n + 1, :Lt], reduction="sum"), z).reshape(C * Lt, C * Lt)
            ggn.append(J.T @ Hz @ J)
        _REFERENCE[key] = (V_ref, ggn)
    return _REFERENCE[key]


def run_backward(model, X, y, lossf, extensions, hook=None):
    model, lossf = extend(model), extend(lossf)
    model.zero_grad()
    loss = lossf(model(X), y)
    with backpack(*extensions, extension_hook=hook):
        loss.backward()
    return loss


def close(a, b, rtol=1e-4, atol=1e-6):
    np.testing.assert_allclose(a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy(), rtol=rtol, atol=atol)


def ggn_close(Vn, want, rtol=1e-4, atol=1e-6):
    """``Vn [V, P]`` (fp32 factor rows of one sample, each entry within ``rtol |v| + atol`` of the truth: the factors' tolerance) ->
    ``Vn^T Vn`` against ``want``: to first order entry (p, q) is off by at most sum_v (dv_p |v_q| + |v_p| dv_q)."""
    Vn = Vn.double()
    A = Vn.abs()
    tol = 2 * rtol * (A.T @ A) + atol * (A.sum(0)[:, None] + A.sum(0)[None, :]) + 1e-12
    err = (Vn.T @ Vn - want).abs()
    assert bool((err <= tol).all()), f"worst error / tolerance = {(err / tol).max().item():.3g}"


def trainable(model):
    return [p for p in model.parameters() if p.requires_grad]


def factors_on(device, subsampling=None, extensions=None, layers=1, frozen=False):
    model, X, y, lossf = make_problem(layers, frozen)
    model, X, y = model.to(device), X.to(device), y.to(device)
    model.set_lengths(list(SRC), list(TGT))
    run_backward(model, X, y, lossf, extensions or [SqrtGGNExact(subsampling=subsampling)])
    return model


def test_the_reference_of_the_padded_batch_is_the_reference_of_the_samples_alone():
    """fp64 against fp64: the two references of this file agree, a sample without targets has no factor, and a sample without a
    source has one only behind the cross-attention."""
    V_ref, ggn = reference()
    model = make_problem()[0]
    assert len(V_ref) == len(list(model.parameters())) and all(float(v.abs().max()) > 1e-3 for v in V_ref)
    Vm = torch.cat([v.flatten(2) for v in V_ref], 2)                                    # [C Tt, N, P]
    for n, (Ls, Lt) in enumerate(zip(SRC, TGT)):
        if Lt == 0:
            assert bool((Vm[:, n] == 0).all())
        elif Ls == 0:
            # (its cross-attention output is rows of zeros: only what comes after still hears of the sample)
            after = {id(p) for p in list(model.head.parameters()) + [model.cross[-1].out_proj.bias]}
            for p, v in zip(model.parameters(), V_ref):
                assert bool((v[:, n] == 0).all()) == (id(p) not in after)
        else:
            G = Vm[:, n].T @ Vm[:, n]
            assert (G - ggn[n]).abs().max().item() <= 1e-11 * max(1.0, ggn[n].abs().max().item())


def test_factors_and_gram_matrix_of_a_padded_batch(device):
    V_ref, ggn = reference()
    model = factors_on(device, extensions=[SqrtGGNExact(), ViViTGGNExact()])
    assert len(V_ref) == len(list(model.parameters()))
    for p, v in zip(model.parameters(), V_ref):
        close(p.sqrt_ggn_exact, v, rtol=1e-4, atol=1e-6)
        gram = oracle.pairwise_dot(v, start_dim=2, flatten=False)                       # [C Tt, N, C Tt, N]
        close(p.vivit_ggn_exact["gram_mat"](), gram, rtol=1e-4, atol=1e-6)
    Vm = torch.cat([p.sqrt_ggn_exact.flatten(2) for p in model.parameters()], 2).cpu()  # [C Tt, N, P]
    for n, want in enumerate(ggn):
        if TGT[n] == 0:
            assert bool((Vm[:, n] == 0).all())
        elif want is not None:
            ggn_close(Vm[:, n], want)
    leaf = model.cross[0].attention
    for kept, given in ((leaf.forward_query_lengths, TGT), (leaf.forward_key_lengths, SRC)):
        assert kept.dtype == torch.int32 and kept.device.type == device.type and kept.tolist() == list(given)


@pytest.mark.parametrize("subsampling", [[0, 0, 1, 3, 1, 2], [2, 0, 1, 3], [2]], ids=["repeated", "permuted", "one"])
def test_subsampling_takes_both_lengths_along(subsampling, device):
    V_ref, _ = reference()
    model = factors_on(device, subsampling)
    for p, v in zip(model.parameters(), V_ref):
        assert p.sqrt_ggn_exact.shape[1] == len(subsampling)
        close(p.sqrt_ggn_exact, v[:, subsampling], rtol=1e-4, atol=1e-6)


def test_a_frozen_memory_skips_the_key_owner(device, monkeypatch):
    """With everything that produces the keys and values frozen (the encoder and the projection of its output: a detached memory) the
    leaf's second input needs no factor: the rule is asked for the query part alone, and the decoder-side factors are those of the
    trainable model."""
    wants = []
    real_kernel, real_torch = kernels.cross_attention_jac_t, ext._cross_attention_jac_t_torch

    def spy_kernel(*a, **k):
        wants.append(("hip", tuple(k["want"])))
        return real_kernel(*a, **k)

    def spy_torch(*a, **k):
        wants.append(("host", tuple(k["want"])))
        return real_torch(*a, **k)

    monkeypatch.setattr(kernels, "cross_attention_jac_t", spy_kernel)
    monkeypatch.setattr(ext, "_cross_attention_jac_t_torch", spy_torch)
    full = factors_on(device)
    flavour = "host" if device.type == "cpu" else "hip"
    assert wants == [(flavour, (True, True))]
    del wants[:]
    model = factors_on(device, frozen=True)
    monkeypatch.undo()
    assert wants == [(flavour, (True, False))]
    V_ref, _ = reference(frozen=True)
    assert len(trainable(model)) == len(V_ref) < len(list(model.parameters()))
    for p, v in zip(trainable(model), V_ref):
        close(p.sqrt_ggn_exact, v, rtol=1e-4, atol=1e-6)
    for p, q in zip(model.parameters(), full.parameters()):
        if p.requires_grad:
            assert torch.equal(p.sqrt_ggn_exact, q.sqrt_ggn_exact)      # the query owner does what it did: the same bytes
        else:
            assert not hasattr(p, "sqrt_ggn_exact")


def test_one_memory_feeds_two_cross_attention_layers(device):
    """The fan-out of the encoder output adds the two layers' contributions."""
    V_ref, _ = reference(layers=2)
    model = factors_on(device, layers=2)
    assert len(V_ref) == len(list(model.parameters()))
    for p, v in zip(model.parameters(), V_ref):
        close(p.sqrt_ggn_exact, v, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("kdim", [None, 6])
@pytest.mark.parametrize("bias", [True, False])
def test_from_torch_reproduces_multihead_attention(bias, kdim):
    torch.manual_seed(3)
    E_, H_, Tq, Tk = 12, 3, 6, 4
    mha = nn.MultiheadAttention(E_, H_, bias=bias, batch_first=True, kdim=kdim, vdim=kdim).double()
    if bias:
        mha.in_proj_bias.data.uniform_(-0.5, 0.5)
        mha.out_proj.bias.data.uniform_(-0.5, 0.5)
    ours = MultiheadCrossAttention.from_torch(mha)
    x, mem = torch.randn(4, Tq, E_, dtype=F64), torch.randn(4, Tk, kdim or E_, dtype=F64)
    ref = mha(x, mem, mem, need_weights=False)[0]
    got = ours(x, mem)
    assert got.shape == ref.shape
    assert ((got - ref).abs().max() / ref.abs().max()).item() <= 1e-12
    for bad in (nn.MultiheadAttention(E_, H_), nn.MultiheadAttention(E_, H_, batch_first=True, dropout=0.1),
                nn.MultiheadAttention(E_, H_, batch_first=True, add_bias_kv=True), nn.MultiheadAttention(E_, H_, batch_first=True, add_zero_attn=True),
                nn.MultiheadAttention(E_, H_, batch_first=True, kdim=6, vdim=5)):
        with pytest.raises(ValueError):
            MultiheadCrossAttention.from_torch(bad)


def test_output_of_another_batch_is_refused(device):
    """The rule reads the forward output from the module; one that does not belong to the inputs is an error."""
    leaf = ScaledDotProductCrossAttention(2).to(device)
    q, kv = torch.rand(3, 4, 4, device=device), torch.rand(3, 5, 8, device=device)
    leaf.inputs, leaf.output = (q, kv), leaf(q, kv)
    M = torch.rand(2, 3, 4, 4, device=device)
    got = ext._cross_attention_jac_t(leaf, M, None, (True, True))
    assert tuple(got[0].shape) == (2, 3, 4, 4) and tuple(got[1].shape) == (2, 3, 5, 8)
    leaf.output = leaf(q[:2], kv[:2])
    with pytest.raises(ValueError, match="does not belong to the queries"):
        ext._cross_attention_jac_t(leaf, M, None, (True, True))


@pytest.mark.gpu
def test_the_encoder_decoder_runs_on_the_hip_kernels(monkeypatch):
    """On the GPU no rule of the model may reach ``torch.autograd.grad`` (the generic input rule), ``torch.einsum`` or
    ``torch.func.vmap``, nor the torch formula of the cross-attention rule: it is a launch of the HIP kernels."""

    def forbidden(*a, **k):
        raise AssertionError("fell back to the torch rule")

    set_kernel_backend(None)
    dev = torch.device("cuda:0")
    V_ref, _ = reference()
    model, X, y, lossf = make_problem()
    model, X, y = model.to(dev), X.to(dev), y.to(dev)
    model.set_lengths(list(SRC), list(TGT))
    monkeypatch.setattr(torch, "einsum", forbidden)
    monkeypatch.setattr(torch.autograd, "grad", forbidden)
    monkeypatch.setattr(torch.func, "vmap", forbidden)
    monkeypatch.setattr(ext, "_cross_attention_jac_t_torch", forbidden)
    run_backward(model, X, y, lossf, [SqrtGGNExact()])
    monkeypatch.undo()
    for p, v in zip(model.parameters(), V_ref):
        close(p.sqrt_ggn_exact, v, rtol=1e-4, atol=1e-6)
