"""Generate golden vectors by running the REFERENCE (f-dangel/vivit @ /root/reference) itself.

Runs only in the build container (the reference does not exist on the GPU box); the resulting
``*.npz`` files hold data only -- seeded inputs and the reference's outputs -- and are committed.

How the reference is made importable:
  * ``Tensor.symeig`` was removed from torch: it is shimmed with ``torch.linalg.eigh/eigvalsh``
    (same semantics: ascending eigenvalues, column eigenvectors, ``upper=True`` default);
  * ``backpack-for-pytorch`` is not installed: an in-memory stub package provides exactly the
    names ``vivit`` imports (savefields ``grad_batch`` / ``sqrt_ggn_exact`` / ``sqrt_ggn_mc`` /
    ``vivit_ggn_exact``).  BackPACK's own factor materialisation is NOT emulated: the factors
    ``V_t`` / ``g`` (and the ViViT closures, built from the reference's own pairwise_dot / Vmp /
    mVp) are hand-made seeded tensors attached to parameters, and the reference's hooks are
    driven exactly as BackPACK would drive them (``hook(module)`` per module).

Usage:  python tests/golden/make_golden.py
        python tests/golden/make_golden.py --gemm-workspace LIB   (gemm_workspace.json only, from the library LIB)
        python tests/golden/make_golden.py --eig-workspace LIB    (eig_workspace.json only, from the library LIB)
"""
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))


def _install_symeig_shim():
    def symeig(self, eigenvectors=False, upper=True):
        uplo = "U" if upper else "L"
        if eigenvectors:
            w, v = torch.linalg.eigh(self, UPLO=uplo)
            return w, v
        return torch.linalg.eigvalsh(self, UPLO=uplo), self.new_empty(0)

    torch.Tensor.symeig = symeig


def _mod(name):
    m = types.ModuleType(name)
    m.__path__ = []
    sys.modules[name] = m
    return m


def _install_backpack_stub():
    bp = _mod("backpack")
    ext = _mod("backpack.extensions")
    bpe = _mod("backpack.extensions.backprop_extension")

    class BackpropExtension:
        def __init__(self, savefield=None, subsampling=None, **kw):
            self.savefield = savefield
            self._subsampling = subsampling

        def get_subsampling(self):
            return self._subsampling

    bpe.BackpropExtension = BackpropExtension

    def _simple(name, savefield):
        def __init__(self, subsampling=None, mc_samples=1):
            BackpropExtension.__init__(self, savefield=savefield, subsampling=subsampling)
            self._mc_samples = mc_samples

        return type(name, (BackpropExtension,), {"__init__": __init__})

    ext.BatchGrad = _simple("BatchGrad", "grad_batch")
    ext.SqrtGGNExact = _simple("SqrtGGNExact", "sqrt_ggn_exact")
    ext.SqrtGGNMC = _simple("SqrtGGNMC", "sqrt_ggn_mc")

    so = _mod("backpack.extensions.secondorder")
    base = _mod("backpack.extensions.secondorder.base")

    class SecondOrderBackpropExtension(BackpropExtension):
        def __init__(self, savefield, fail_mode, module_exts, subsampling=None):
            BackpropExtension.__init__(self, savefield=savefield, subsampling=subsampling)

    base.SecondOrderBackpropExtension = SecondOrderBackpropExtension
    hbp = _mod("backpack.extensions.secondorder.hbp")

    class LossHessianStrategy:
        EXACT = "exact"
        SAMPLING = "sampling"

    hbp.LossHessianStrategy = LossHessianStrategy
    sq = _mod("backpack.extensions.secondorder.sqrt_ggn")

    class _Any:
        def __init__(self, *a, **k):
            pass

    class _AnyModule(types.ModuleType):
        def __getattr__(self, item):
            if item.startswith("__"):
                raise AttributeError(item)
            return _Any

    for sub in ["activations", "custom_module", "dropout", "flatten", "losses", "pad", "padding", "pooling", "slicing"]:
        m = _AnyModule(f"backpack.extensions.secondorder.sqrt_ggn.{sub}")
        sys.modules[m.__name__] = m
        setattr(sq, sub, m)
    mm = _mod("backpack.extensions.mat_to_mat_jac_base")

    class MatToJacMat:
        def __init__(self, derivatives, params=None):
            self.derivatives = derivatives

    mm.MatToJacMat = MatToJacMat
    _mod("backpack.core")
    _mod("backpack.core.derivatives")
    for sub, names in {
        "basederivatives": ["BaseDerivatives"],
        "linear": ["LinearDerivatives"],
        "conv1d": ["Conv1DDerivatives"],
        "conv2d": ["Conv2DDerivatives"],
        "conv3d": ["Conv3DDerivatives"],
        "conv_transpose1d": ["ConvTranspose1DDerivatives"],
        "conv_transpose2d": ["ConvTranspose2DDerivatives"],
        "conv_transpose3d": ["ConvTranspose3DDerivatives"],
        "batchnorm_nd": ["BatchNormNdDerivatives"],
    }.items():
        m = _mod(f"backpack.core.derivatives.{sub}")
        for n in names:
            setattr(m, n, type(n, (), {"__init__": lambda self, *a, **k: None}))
    _mod("backpack.custom_module")
    for sub, names in {
        "branching": ["SumModule", "Parallel"],
        "pad": ["Pad"],
        "scale_module": ["ScaleModule"],
        "slicing": ["Slicing"],
    }.items():
        m = _mod(f"backpack.custom_module.{sub}")
        for n in names:
            setattr(m, n, type(n, (torch.nn.Module,), {}))
    _mod("backpack.utils")
    ss = _mod("backpack.utils.subsampling")

    def subsample(tensor, dim=0, subsampling=None):
        if subsampling is None:
            return tensor
        return tensor.index_select(dim, torch.tensor(subsampling))

    ss.subsample = subsample
    hf = _mod("backpack.hessianfree")
    for sub in ["ggnvp", "hvp"]:
        m = _AnyModule(f"backpack.hessianfree.{sub}")
        sys.modules[m.__name__] = m
    cp = _AnyModule("backpack.utils.convert_parameters")
    sys.modules[cp.__name__] = cp
    return bp


def import_reference():
    _install_symeig_shim()
    _install_backpack_stub()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import vivit  # noqa: F401  (the real reference package)

    assert vivit.__file__.startswith(REF), vivit.__file__
    return vivit


class FakeModule(torch.nn.Module):
    """A leaf module holding parameters and the ``input0`` BackPACK stores (linalg/utils.py:54)."""

    def __init__(self, params, batch_size):
        super().__init__()
        for i, p in enumerate(params):
            self.register_parameter(f"p{i}", p)
        self.input0 = torch.zeros(batch_size, 1)


def make_factors(seed, C, N, shapes, N_grad=None, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    V = [torch.randn(C, N, *s, generator=g, dtype=dtype) / (N**0.5) for s in shapes]
    G = [torch.randn(N_grad or N, *s, generator=g, dtype=dtype) / (N_grad or N) for s in shapes]
    return V, G


def top_k_criterion(k, must_exceed=1e-5):
    """Same rule as the reference tests' make_criterion (test/optim/settings.py:21-47)."""

    def criterion(evals):
        n = len(evals)
        shift = max(n - k, 0)
        return [i + shift for i, ev in enumerate(evals[shift:]) if ev > must_exceed]

    return criterion


def keep_all(evals):
    return list(range(evals.numel()))


def constant_damping(d):
    def damping(evals, evecs, gammas, lambdas):
        return d * torch.ones_like(evals)

    return damping


CASES = [
    # name, C, N, param shapes, N_grad, batch_size N_total, criterion, k
    dict(name="mlp_small", seed=1, C=3, N=4, shapes=[(5, 7), (5,)], k=2),
    dict(name="conv_like", seed=2, C=5, N=3, shapes=[(2, 3, 2, 2), (2,), (4, 6), (4,)], k=10),
    dict(name="subsampled", seed=3, C=4, N=2, shapes=[(6, 5), (6,)], k=3, N_total=6, N_grad=3),
    dict(name="mc1", seed=4, C=1, N=8, shapes=[(4, 9), (4,), (3, 4)], k=4),
    dict(name="wide", seed=5, C=10, N=6, shapes=[(12, 20), (12,)], k=10),
    # n = C*N = 320 > 192: the multi-kernel eigensolver (tridiagonalisation + D&C + back-transformation) instead of
    # the single-workgroup one that serves the reference's own test sizes
    dict(name="multikernel", seed=6, C=10, N=32, shapes=[(16, 24), (16,)], k=10),
]
# n = C*N = 2560 > 2048: the two-stage eigensolver the headline runs (band reduction, bulge chase, divide & conquer, Q2, Q1).
# The factors are 30 MB: only their SEED is stored (tests/helpers.py:planted_factors regenerates them in the test -- the build
# container and the GPU box run the same torch, whose CPU generator is deterministic) together with the reference's outputs.
BIG_CASES = [
    dict(name="two_stage", seed=8, C=10, N=256, shapes=[(48, 60), (48,)], k=10),
]


def run_case(vivit, case):
    from vivit.utils.ggn import Vmp
    from vivit.utils.gram import mVp, pairwise_dot, partial_contract

    C, N, shapes = case["C"], case["N"], case["shapes"]
    N_total = case.get("N_total", N)
    N_grad = case.get("N_grad", N_total)
    V, G = make_factors(case["seed"], C, N, shapes, N_grad=N_grad)
    out = {"C": C, "N": N, "N_total": N_total, "N_grad": N_grad, "k": case["k"]}
    for i, (v, g) in enumerate(zip(V, G)):
        out[f"V{i}"] = v.numpy()
        out[f"g{i}"] = g.numpy()
    subsampling = None if N_total == N else list(range(N))
    sub_grad = None if N_grad == N_total else list(range(N_grad))

    # --- raw contractions (K1, K2, K8, K9) straight from vivit/utils/{gram,ggn}.py
    out["gram_flat"] = sum(pairwise_dot(v, start_dim=2) for v in V).numpy()
    out["V_t_g0"] = partial_contract(V[0], G[0], (2, 1)).numpy()
    gen = torch.Generator().manual_seed(99)
    mat = torch.randn(3, C, N, generator=gen)
    out["mat"] = mat.numpy()
    out["Vmp0"] = Vmp(V[0], mat, 2).numpy()
    pm = torch.randn(2, *shapes[0], generator=gen)
    out["pmat"] = pm.numpy()
    out["mVp0"] = mVp(V[0], pm, 2).numpy()

    def fresh_params():
        return [torch.nn.Parameter(torch.zeros(*s)) for s in shapes]

    # --- parameter-list forms: compute_gram_mat, V_mat_prod(concat), sqrt_gram_mat_prod(concat)
    from vivit.utils.ggn import V_mat_prod
    from vivit.utils.gram import compute_gram_mat, sqrt_gram_mat_prod

    params = fresh_params()
    for p_, v in zip(params, V):
        p_.sqrt_factor = v
    out["compute_gram_mat"] = compute_gram_mat(params, "sqrt_factor", 2, flatten=True).numpy()
    out["V_mat_prod_concat"] = V_mat_prod(mat, params, "sqrt_factor", concat=True).numpy()
    for i, r in enumerate(V_mat_prod(mat, params, "sqrt_factor")):
        out[f"V_mat_prod{i}"] = r.numpy()
    sub_idx = [N - 1, 0]  # sub-sampled application: V_t[:, subsampling] (vivit/utils/ggn.py:53-70)
    out["V_mat_prod_sub0"] = V_mat_prod(mat[:, :, :2].contiguous(), params, "sqrt_factor", subsampling=sub_idx)[0].numpy()
    cmat = torch.randn(C * N, 3, generator=gen)
    out["cmat"] = cmat.numpy()
    out["sqrt_gram_mat_prod_concat"] = sqrt_gram_mat_prod(cmat, params, "sqrt_factor", 2, concat=True).numpy()
    for i, r in enumerate(sqrt_gram_mat_prod(cmat, params, "sqrt_factor", 2)):
        out[f"sqrt_gram_mat_prod{i}"] = r.numpy()

    # --- EigvalshComputation / EighComputation (closures built from the reference's own utils)
    def attach_vivit(params, savefield):
        for p, v in zip(params, V):
            setattr(
                p,
                savefield,
                {
                    "gram_mat": (lambda v=v: pairwise_dot(v, start_dim=2, flatten=False)),
                    "V_mat_prod": (lambda m, v=v: Vmp(v, m, 2)),
                    "V_t_mat_prod": (lambda m, v=v: mVp(v, m, 2)),
                },
            )

    for groups_kind in ["one", "per_param"]:
        params = fresh_params()
        comp = vivit.EigvalshComputation(subsampling=subsampling)
        attach_vivit(params, "vivit_ggn_exact")
        groups = [{"params": params}] if groups_kind == "one" else [{"params": [p]} for p in params]
        hook = comp.get_extension_hook(groups)
        hook(FakeModule(params, N_total))
        for gi, grp in enumerate(groups):
            out[f"eigvalsh_{groups_kind}_{gi}"] = comp.get_result(grp).numpy()

    params = fresh_params()
    comp = vivit.EighComputation(subsampling=subsampling, warn_small_eigvals=0.0)
    attach_vivit(params, "vivit_ggn_exact")
    crit = top_k_criterion(case["k"])
    groups = [{"params": params, "criterion": crit}]
    comp.get_extension_hook(groups)(FakeModule(params, N_total))
    evals, evecs = comp.get_result(groups[0])
    out["eigh_evals"] = evals.numpy()
    for i, e in enumerate(evecs):
        out[f"eigh_evecs{i}"] = e.numpy()

    # --- DirectionalDerivatives / DirectionalDampedNewton on materialised factors
    mc = 1 if case["name"].startswith("mc") else 0
    savefield_ggn = "sqrt_ggn_mc" if mc else "sqrt_ggn_exact"

    def attach_sqrt(params):
        for p, v, g in zip(params, V, G):
            setattr(p, savefield_ggn, v.clone())
            p.grad_batch = g.clone()

    params = fresh_params()
    comp = vivit.DirectionalDerivativesComputation(
        subsampling_grad=sub_grad, subsampling_ggn=subsampling, mc_samples_ggn=mc, warn_small_eigvals=0.0
    )
    attach_sqrt(params)
    groups = [{"params": params, "criterion": crit}]
    comp.get_extension_hook(groups)(FakeModule(params, N_total))
    gammas, lambdas = comp.get_result(groups[0])
    out["gammas"] = gammas.numpy()
    out["lambdas"] = lambdas.numpy()

    params = fresh_params()
    comp = vivit.DirectionalDampedNewtonComputation(
        subsampling_grad=sub_grad, subsampling_ggn=subsampling, mc_samples_ggn=mc, warn_small_eigvals=0.0
    )
    attach_sqrt(params)
    groups = [{"params": params, "criterion": crit, "damping": constant_damping(1.0)}]
    comp.get_extension_hook(groups)(FakeModule(params, N_total))
    for i, s in enumerate(comp.get_result(groups[0])):
        out[f"newton{i}"] = s.numpy()

    # --- GramSqrtGGN hook (stand-alone Gram, K1 + accumulation)
    from vivit.extensions.hooks import GramBatchGrad, CenteredGramBatchGrad, GramSqrtGGNExact, GramSqrtGGNMC

    params = fresh_params()
    attach_sqrt(params)
    hook = (GramSqrtGGNMC if mc else GramSqrtGGNExact)()
    hook(FakeModule(params, N_total))
    out["gram_hook"] = hook.get_result().numpy()
    for cls, key in [(GramBatchGrad, "gram_batch_grad"), (CenteredGramBatchGrad, "gram_batch_grad_centered")]:
        params = fresh_params()
        attach_sqrt(params)
        hook = cls()
        hook(FakeModule(params, N_total))
        out[key] = hook.get_result().numpy()
    from vivit.extensions.hooks import CenteredBatchGrad

    params = fresh_params()
    attach_sqrt(params)
    hook = CenteredBatchGrad()
    hook(FakeModule(params, N_total))
    for i, p_ in enumerate(params):
        out[f"centered_grad_batch{i}"] = getattr(p_, hook.savefield).numpy()
    return out


def run_big_case(vivit, case):
    """EigvalshComputation, EighComputation (top k) and the directional derivatives / damped Newton step of the reference
    on seeded factors that are NOT stored (see BIG_CASES)."""
    from vivit.utils.ggn import Vmp
    from vivit.utils.gram import mVp, pairwise_dot

    sys.path.insert(0, os.path.dirname(OUT))
    from helpers import planted_factors   # the seeded recipe the tests regenerate the factors with (data, no product code)

    C, N, shapes = case["C"], case["N"], case["shapes"]
    V, G = planted_factors(case["seed"], C, N, shapes)
    out = {"C": C, "N": N, "N_total": N, "N_grad": N, "k": case["k"], "seed": case["seed"],
           "shapes_flat": np.array([d for s in shapes for d in (len(s),) + tuple(s)]),
           # fingerprints of the regenerated factors (a torch whose generator differs must fail loudly, not subtly)
           "V_checksum": np.array([float(v.double().sum()) for v in V] + [float(v.double().abs().sum()) for v in V]),
           "g_checksum": np.array([float(g.double().sum()) for g in G] + [float(g.double().abs().sum()) for g in G])}

    def fresh_params():
        return [torch.nn.Parameter(torch.zeros(*s)) for s in shapes]

    def attach_vivit(params):
        for p, v in zip(params, V):
            p.vivit_ggn_exact = {"gram_mat": (lambda v=v: pairwise_dot(v, start_dim=2, flatten=False)),
                                 "V_mat_prod": (lambda m, v=v: Vmp(v, m, 2)), "V_t_mat_prod": (lambda m, v=v: mVp(v, m, 2))}

    def attach_sqrt(params):
        for p, v, g in zip(params, V, G):
            p.sqrt_ggn_exact = v.clone()
            p.grad_batch = g.clone()

    params = fresh_params()
    comp = vivit.EigvalshComputation()
    attach_vivit(params)
    groups = [{"params": params}]
    comp.get_extension_hook(groups)(FakeModule(params, N))
    out["eigvalsh_one_0"] = comp.get_result(groups[0]).numpy()

    crit = top_k_criterion(case["k"])
    params = fresh_params()
    comp = vivit.EighComputation(warn_small_eigvals=0.0)
    attach_vivit(params)
    groups = [{"params": params, "criterion": crit}]
    comp.get_extension_hook(groups)(FakeModule(params, N))
    evals, evecs = comp.get_result(groups[0])
    out["eigh_evals"] = evals.numpy()
    for i, e in enumerate(evecs):
        out[f"eigh_evecs{i}"] = e.numpy()

    params = fresh_params()
    comp = vivit.DirectionalDerivativesComputation(warn_small_eigvals=0.0)
    attach_sqrt(params)
    groups = [{"params": params, "criterion": crit}]
    comp.get_extension_hook(groups)(FakeModule(params, N))
    gammas, lambdas = comp.get_result(groups[0])
    out["gammas"], out["lambdas"] = gammas.numpy(), lambdas.numpy()

    params = fresh_params()
    comp = vivit.DirectionalDampedNewtonComputation(warn_small_eigvals=0.0)
    attach_sqrt(params)
    groups = [{"params": params, "criterion": crit, "damping": constant_damping(1.0)}]
    comp.get_extension_hook(groups)(FakeModule(params, N))
    for i, s in enumerate(comp.get_result(groups[0])):
        out[f"newton{i}"] = s.numpy()
    return out


def run_eig_utils(vivit):
    """vivit/utils/eig.py on the matrices of test/utils/test_stable_symeig.py:10-11 plus a PSD one."""
    from vivit.utils.eig import shift_diag, symeig, symeig_psd

    out = {}
    T1 = torch.diag(torch.Tensor([1.1, 2.2, 9.9]))
    T2 = torch.Tensor([[1.1, 2.2, 3.3], [4.4, 5.5, 6.6], [7.7, 8.8, 2.2]])
    g = torch.Generator().manual_seed(7)
    B = torch.randn(6, 3, generator=g)
    T3 = B @ B.T  # rank 3 of 6 -> zero eigenvalues to filter
    for name, T in [("T1", T1), ("T2", T2), ("T3", T3)]:
        out[name] = T.numpy()
        for shift in [0.0, 0.1, 1.0, 10.0]:
            w, v = symeig_psd(T.clone(), eigenvectors=True, shift=shift)
            out[f"{name}_psd_w_{shift}"] = w.numpy()
        w, v = symeig(T.clone(), eigenvectors=True)
        out[f"{name}_symeig_w"] = w.numpy()
        out[f"{name}_symeig_nvec"] = np.array(v.shape[1] if v.numel() else 0)
    inp = torch.tensor([[1.0, 1.0], [2.0, 2.0], [3.0, 4.0]])
    out["shift_nonsquare"] = shift_diag(inp, 0.1).numpy()
    return out


# ---- workspace sizes of the GEMM routes (tests/test_gemm_plan_host.py): no reference involved, data recorded from a BUILT
# libvivit_hip.so -- the one of the commit BEFORE a change to the launch planning of the GEMM routes (csrc/gemm_plan.h), so that the change
# can be held to "every query answers what it answered before".  Default environment (no VIVIT_GEMM* switch set).
def _gemm_workspace_shapes():
    """(m, n, k) of vivit_gemm_f32_workspace_bytes and (n, p) of vivit_gram_syrk_f32_workspace_bytes on both sides of every
    route boundary of the planner (tile counts that are prime, such as 199 and 101, have no shape with M, N >= 256: the nearest
    products stand in)."""
    gemm, syrk = [], []
    # 256-tile plan: 200 tiles (10 x 20, 8 x 25) against 198 (11 x 18), 196, 195; K 511 | 512; M, N 511 | 512; split-K depths
    for m, n in ((2560, 5120), (2048, 6400), (2816, 4608), (3584, 3584), (3328, 3840), (511, 102400), (512, 102400), (4096, 4096)):
        for k in (496, 511, 512, 527, 2064, 2071, 4096, 8192, 16384, 65536, 401408):
            gemm.append((m, n, k))
    for n in (4864, 4865, 5120, 40960):          # 19 | 20 tile rows: 190 | 210 lower tiles
        for p in (511, 512, 2048, 4096, 4100, 65536, 401408):
            syrk.append((n, p))
    # bf16-pipe split-K: K 16368 | 16384, 100 tiles (10 x 10) | 102 (6 x 17) | 101 columns of one tile row, M, N 255 | 256
    for m, n in ((2560, 2560), (1536, 4352), (256, 25600), (256, 25856), (255, 2560), (256, 2560), (2560, 255), (1000, 1300), (1280, 1280)):
        for k in (16368, 16383, 16384, 20480, 131072, 401408):
            gemm.append((m, n, k))
    for n in (255, 256, 1280, 3328, 3329, 3584):   # 13 | 14 | 15 tile rows: 91 | 105 lower tiles
        for p in (16368, 16384, 20480, 401408):
            syrk.append((n, p))
    # 64-row streaming route: M 64 | 65, N 2047 | 2048, K 2047 | 2048 and K % 16 != 0
    for m in (1, 4, 17, 64, 65):
        for n in (2047, 2048, 2304, 40960):
            for k in (2032, 2047, 2048, 4096, 4100, 65536):
                gemm.append((m, n, k))
    # deep-K small-output route: N 1024 | 1025, K 2047 | 2048, K % 4 != 0
    for m in (17, 48, 64, 65):
        for n in (64, 700, 1024, 1025):
            for k in (2047, 2048, 2050, 8190, 8192, 40960):
                gemm.append((m, n, k))
    # 128-tile split-K: fewer than 256 tiles with 63 | 64 K tiles; 256 tiles; one tile row
    for m, n in ((300, 300), (128, 128), (2048, 2048), (1920, 2048), (64, 129), (17, 128)):
        for k in (1008, 1009, 1024, 5001, 40960):
            gemm.append((m, n, k))
    # the route cases of tests/gemm_contract_child.py and the headline Gram build
    gemm += [(4096, 4096, 2064), (4096, 4096, 2071), (1000, 1300, 20480), (64, 2304, 4096), (1, 2048, 2048), (48, 700, 8192),
             (8, 5000, 3000), (300, 300, 5001)]
    syrk += [(40960, 401408), (512, 2048), (300, 500)]
    return sorted(set(gemm)), sorted(set(syrk))


def gemm_workspace_table(lib_path):
    import ctypes
    import json

    lib = ctypes.CDLL(lib_path)
    for f in (lib.vivit_gemm_f32_workspace_bytes, lib.vivit_gram_syrk_f32_workspace_bytes):
        f.restype = ctypes.c_size_t
    lib.vivit_gemm_f32_workspace_bytes.argtypes = [ctypes.c_int64] * 3
    lib.vivit_gram_syrk_f32_workspace_bytes.argtypes = [ctypes.c_int64] * 2
    assert not [v for v in os.environ if v.startswith("VIVIT_GEMM") or v == "VIVIT_BX_ASM"], "default environment only"
    gemm, syrk = _gemm_workspace_shapes()
    table = {"gemm": [[m, n, k, lib.vivit_gemm_f32_workspace_bytes(m, n, k)] for m, n, k in gemm],
             "syrk": [[n, p, lib.vivit_gram_syrk_f32_workspace_bytes(n, p)] for n, p in syrk]}
    with open(os.path.join(OUT, "gemm_workspace.json"), "w") as f:
        f.write("{\n" + ",\n".join('"%s": [\n%s\n]' % (k, ",\n".join(json.dumps(r) for r in v)) for k, v in table.items()) + "\n}\n")
    print("gemm_workspace.json:", len(gemm), "GEMM shapes,", len(syrk), "SYRK shapes")


# ---- workspace sizes of the eigensolver entries (tests/test_eig_workspace_host.py): recorded, like the GEMM table, from the
# BUILT library of the commit before the eigensolver workspaces got one layout function each.  The route switches are read
# once per process, so every environment is asked in a process of its own.
EIG_WORKSPACE_ENVS = {"unset": None, "0": "0", "1": "1"}   # VIVIT_TWO_STAGE, each with VIVIT_SYTRD_PERSIST=0
_EIG_QUERY_ARGS = {"vivit_symeig_f32": 2, "vivit_symeigvals_batched_f32": 2, "vivit_symeig_reduce_f32": 1, "vivit_symeig_select_f32": 2,
                   "vivit_symeig_select_batched_f32": 3, "vivit_sytrd_f32": 1, "vivit_stedc_f32": 2, "vivit_sy2sb_f32": 1,
                   "vivit_sy2sb_panel_qr_f32": 1, "vivit_sb2st_f32": 1, "vivit_q2_apply_f32": 1}


def _eig_workspace_rows():
    """[entry, args...] of every public eigensolver query on both sides of every boundary the layouts branch on."""
    sizes = [128, 129, 192, 193, 200, 300, 512, 1280, 1281, 2047, 2048, 2049, 4095, 4096, 4097, 4100, 8191, 8192, 16383, 16384,
             40960]
    rows = []
    for n in sizes:
        rows += [["vivit_symeig_f32", n, 0], ["vivit_symeig_f32", n, 1], ["vivit_symeig_reduce_f32", n], ["vivit_sytrd_f32", n],
                 ["vivit_stedc_f32", n, 0], ["vivit_stedc_f32", n, 1], ["vivit_sy2sb_f32", n], ["vivit_sy2sb_panel_qr_f32", n],
                 ["vivit_sb2st_f32", n], ["vivit_q2_apply_f32", n]]
        for K in (1, 256, 257, n):
            rows.append(["vivit_symeig_select_f32", n, K])
        for batch in (1, 7, 8, 9):
            rows.append(["vivit_symeigvals_batched_f32", n, batch])
            for K in (1, 256, 257, n):
                rows.append(["vivit_symeig_select_batched_f32", n, batch, K])
    rows.append(["vivit_sy2sb_panel_qr_f32", 100])
    return rows


def eig_workspace_answers(lib_path, rows):
    """rows with the library's answer appended (this process's environment)."""
    import ctypes

    lib = ctypes.CDLL(lib_path)
    out = []
    for name, *args in rows:
        f = getattr(lib, name + "_workspace_bytes")
        f.restype = ctypes.c_size_t
        f.argtypes = [ctypes.c_int64] * _EIG_QUERY_ARGS[name]
        if name in ("vivit_symeig_f32", "vivit_stedc_f32"):
            f.argtypes = [ctypes.c_int64, ctypes.c_int]
        out.append([name] + args + [f(*args)])
    return out


def eig_workspace_env(two_stage):
    env = {k: v for k, v in os.environ.items() if not k.startswith("VIVIT_")}
    env["VIVIT_SYTRD_PERSIST"] = "0"
    if two_stage is not None:
        env["VIVIT_TWO_STAGE"] = two_stage
    return env


def eig_workspace_table(lib_path):
    import json
    import subprocess

    table = {}
    for key, two_stage in EIG_WORKSPACE_ENVS.items():
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--eig-workspace-rows", lib_path], env=eig_workspace_env(two_stage),
                             stdout=subprocess.PIPE, check=True, text=True).stdout
        table[key] = json.loads(out.strip().splitlines()[-1])
    with open(os.path.join(OUT, "eig_workspace.json"), "w") as f:
        f.write("{\n" + ",\n".join('"%s": [\n%s\n]' % (k, ",\n".join(json.dumps(r) for r in v)) for k, v in table.items()) + "\n}\n")
    print("eig_workspace.json:", len(table), "environments,", len(table["unset"]), "queries each")


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--eig-workspace":   # python make_golden.py --eig-workspace path/to/libvivit_hip.so
        return eig_workspace_table(sys.argv[2])
    if len(sys.argv) == 3 and sys.argv[1] == "--eig-workspace-rows":   # (the child of --eig-workspace: one environment)
        import json
        return print(json.dumps(eig_workspace_answers(sys.argv[2], _eig_workspace_rows())))
    if len(sys.argv) == 3 and sys.argv[1] == "--gemm-workspace":   # python make_golden.py --gemm-workspace path/to/libvivit_hip.so
        return gemm_workspace_table(sys.argv[2])
    vivit = import_reference()
    for case in CASES:
        res = run_case(vivit, case)
        np.savez_compressed(os.path.join(OUT, f"{case['name']}.npz"), **res)
        print(case["name"], {k: getattr(v, "shape", v) for k, v in list(res.items())[:4]}, "...", len(res), "arrays")
    for case in BIG_CASES:
        res = run_big_case(vivit, case)
        np.savez_compressed(os.path.join(OUT, f"{case['name']}.npz"), **res)
        print(case["name"], len(res), "arrays,", sum(v.nbytes for v in res.values() if hasattr(v, "nbytes")), "bytes")
    np.savez_compressed(os.path.join(OUT, "eig_utils.npz"), **run_eig_utils(vivit))
    print("wrote", sorted(f for f in os.listdir(OUT) if f.endswith(".npz")))


if __name__ == "__main__":
    main()
