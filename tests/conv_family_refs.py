"""fp64 references, fp64 stand-ins for the four 2-D entry points, and the case list for the LOWERINGS of the convolution
family in vivit_amd/backend/extensions.py: Conv1d, grouped Conv2d, Conv3d, ConvTranspose1d/2d/3d, Max/AvgPool1d and
Max/AvgPool3d on ``kernels.conv2d_weight_mjp``, ``kernels.conv2d_jac_t``, ``kernels.maxpool2d_jac_t`` and
``kernels.avgpool2d_jac_t``.  TEST INFRASTRUCTURE: a plain module shared by tests/test_conv_family_refs_host.py (no GPU),
tests/test_conv_family_gpu.py and its child tests/conv_family_child.py.  The two Conv2d kernels themselves are pinned by
tests/conv_refs.py; this module is about the index arithmetic above them (``_depth_range``, the stacked tall image of
``_conv3d_weight_contract``, the tap flip and the group slices of ``_convtranspose2d_input``, the separable pooling).

References: torch's functional ops in fp64 on the CPU.  Input rule: batched autograd of F.conv{1,2,3}d /
F.conv_transpose{1,2,3}d / F.avg_pool{1,3}d.  Weight rule: per sample, autograd with respect to the weight.  MaxPool: an
explicit selection (:func:`maxpool_first_max`) of the FIRST maximum of every window in d-major scan order, which is what
the docstring of ``_hip_pool3d_jac_t`` claims of the separable composition -- no device's tie-breaking enters.

Stand-ins (:class:`StandIns`): the four wrappers in fp64 with the wrappers' signatures.  They take what the entry points
take -- in particular an ``OH`` / ``OW`` read off ``M`` that is SMALLER than the floor formula of the image (a transposed
layer's ``output_padding``, the ``tail`` rows of the stack): the extra image rows and columns are simply never read.  The
two convolution stand-ins assert the geometry check of the .hip files, ``(OH - 1) s + (K - 1) d - p < H + p``, and nothing
stricter.  Every call is recorded with its 2-D geometry, so that the host test can label it with the planner mirrors of
tests/conv_refs.py.

Input families (tests/epilogue_refs.py):
* exact: integers from {-4..4}.  Every term is an integer of magnitude <= 16 and every partial sum an integer below 2^24
  (:func:`reference` returns ``sum|terms|``; the host test asserts the maximum for every case), so the fp32 result must equal
  the fp64 reference BIT FOR BIT whatever the order, across depth taps as well.  AvgPool multiplies by 1 / (kh kw) and then
  by 1 / kd: exact cases have windows whose two factors are powers of two, every other window is generic only.
* generic: seeded randn over three orders of magnitude, under the elementwise bound (n + 2) eps sum|terms| (:func:`n_terms`).
  Derivation: a sum evaluated as ANY tree of fp32 additions of exact products (an FMA chain, the matrix pipe, a split over
  waves) has error <= depth eps sum|terms| to first order, and the depth is at most the number of leaves; the + 2 covers the
  second-order terms (n eps < 1e-4 here).
  - input rule, served by the kernel: one 2-D launch adds Cout/G KH KW terms into an entry (structural zeros of the stride
    included), and the 3-D lowerings then add the KD tap results with ``g[...] += res``: n = Cout/G KH KW + KD.
  - input rule through the generic rule (``served is None``, or the matrix pipe switched off): torch's own backward, order
    unknown: n = Cout/G KD KH KW, all terms of the entry.
  - weight rule: one launch contracts over the coefficient's positions, n = OH OW; for the 3-D rule those are the rows of the
    stack INCLUDING the zero rows behind every slice, n = QD (QH + ceil((KH - 1) dh / sh)) QW.  (The taps are stacked, not
    added.)
  - MaxPool: an entry collects the cotangents of the windows that selected it, at most kh kw in the plane stage of at most
    kd each from the depth stage: n = kd + kh kw.
  - AvgPool: as MaxPool, and each stage multiplies its sum by the ROUNDED reciprocal of the window (two roundings per
    stage): n = kd + kh kw + 4 (n = k + 2 in one dimension).
  No constant here is measured.

``_convtranspose2d_input`` has three reasons to return ``None``.  ``p > (K - 1) d`` and ``Cout/G kh kw > 1024`` have cases.
The third, ``full < (q - 1) s + 1``, is NOT reachable from a module: ``M`` has the layer's output size H' = (q - 1) s - 2 p +
d (K - 1) + op + 1, so full = H' + 2 p - d (K - 1) = (q - 1) s + op + 1 >= (q - 1) s + 1.  No case.

``hrows < H`` in ``_conv3d_weight_contract`` is not reachable from a Conv3d either: QH sh >= H + 2 ph - (KH - 1) dh and the
zero rows add at least (KH - 1) dh, so the pitch minus ph is at least H + ph.  (KH = 1, sh = 3 leaves trailing rows unread,
case "c3-unread-rows", but they still lie inside the slice.)  It takes a ConvTranspose3d with output_padding >= stride +
padding, which torch admits when the dilation exceeds the stride: case "t3-hrows".
"""
import functools
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as F
from torch import nn

import conv_refs as R
from epilogue_refs import EPS, exact, generic, misaligned  # noqa: F401  (re-exported for the tests)

F64 = torch.float64
FAMILIES = ("exact", "generic")
V_SLICES, N_BATCH = R.V_SLICES, R.N_BATCH

Case = namedtuple("Case", "name kind spec expects")

NDIM = {"conv1d": 1, "conv2d": 2, "conv3d": 3, "convT1d": 1, "convT2d": 2, "convT3d": 3, "maxpool1d": 1, "avgpool1d": 1,
        "maxpool3d": 3, "avgpool3d": 3}
CONV_FN = {"conv1d": F.conv1d, "conv2d": F.conv2d, "conv3d": F.conv3d, "convT1d": F.conv_transpose1d,
           "convT2d": F.conv_transpose2d, "convT3d": F.conv_transpose3d}
MODULE = {"conv1d": nn.Conv1d, "conv2d": nn.Conv2d, "conv3d": nn.Conv3d, "convT1d": nn.ConvTranspose1d,
          "convT2d": nn.ConvTranspose2d, "convT3d": nn.ConvTranspose3d, "maxpool1d": nn.MaxPool1d, "avgpool1d": nn.AvgPool1d,
          "maxpool3d": nn.MaxPool3d, "avgpool3d": nn.AvgPool3d}


def tup(v, n):
    return (v,) * n if isinstance(v, int) else tuple(v)


def is_conv(kind):
    return kind.startswith("conv")


def is_transposed(kind):
    return kind.startswith("convT")


def is_max(kind):
    return kind.startswith("maxpool")


def rules_of(case):
    return ("input", "weight") if is_conv(case.kind) else ("input",)


def families_of(case):
    return case.expects.get("families", FAMILIES)


# ---- geometry of a case ---------------------------------------------------------------------------------------------------
def conv_kwargs(case):
    """stride / padding / dilation / groups (/ output_padding) of a convolution case as tuples."""
    n, s = NDIM[case.kind], case.spec
    kw = dict(stride=tup(s.get("s", 1), n), padding=tup(s.get("p", 0), n), dilation=tup(s.get("d", 1), n), groups=s.get("g", 1))
    if is_transposed(case.kind):
        kw["output_padding"] = tup(s.get("op", 0), n)
    return kw


def pool_kwargs(case):
    """The module's keyword arguments of a pooling case (kernel_size, stride, padding as tuples, the rest as given)."""
    n, s = NDIM[case.kind], case.spec
    k = tup(s["k"], n)
    kw = dict(kernel_size=k, stride=tup(s.get("s", k), n), padding=tup(s.get("p", 0), n))
    kw.update({key: s[key] for key in ("ceil_mode", "dilation", "count_include_pad", "divisor_override") if key in s})
    return kw


def weight_shape(case):
    s, n = case.spec, NDIM[case.kind]
    g = s.get("g", 1)
    lead = (s["cin"], s["cout"] // g) if is_transposed(case.kind) else (s["cout"], s["cin"] // g)
    return lead + tup(s["k"], n)


def in_shape(case):
    s = case.spec
    return (s.get("N", N_BATCH), s["cin"] if is_conv(case.kind) else s["c"]) + tup(s["size"], NDIM[case.kind])


def forward(case, x, W=None):
    """The layer of a case by torch's functional op."""
    if is_conv(case.kind):
        return CONV_FN[case.kind](x, W, None, **conv_kwargs(case))
    fn = {"maxpool1d": F.max_pool1d, "avgpool1d": F.avg_pool1d, "maxpool3d": F.max_pool3d, "avgpool3d": F.avg_pool3d}[case.kind]
    return fn(x, **pool_kwargs(case))


@functools.lru_cache(maxsize=None)
def _out_shape(case_key):
    case = ALL[case_key]
    x = torch.zeros(in_shape(case), dtype=F64)
    W = torch.zeros(weight_shape(case), dtype=F64) if is_conv(case.kind) else None
    return tuple(forward(case, x, W).shape)


def out_shape(case):
    """[N, C, *spatial] of the layer's output (read off torch's own forward)."""
    return _out_shape(case.name)


def make_module(case, W=None):
    """The torch module of a case (CPU, fp32; bias-free), its weight set to ``W``."""
    if is_conv(case.kind):
        s = case.spec
        m = MODULE[case.kind](s["cin"], s["cout"], tup(s["k"], NDIM[case.kind]), bias=False, **conv_kwargs(case))
        if W is not None:
            m.weight.data = W.clone()
        return m
    return MODULE[case.kind](**pool_kwargs(case))


# ---- operands ---------------------------------------------------------------------------------------------------------------
def _pool_input(case, fam, gen, shape):
    """The input of a pooling case.  Maximum pooling selects by it: "ties" is floor(3 rand) (a third of a window shares
    the maximum), "equal" one value per (n, c, d) plane, and otherwise the values are all DISTINCT (integers for the exact
    family), so that the cases that ride torch's own backward do not depend on its tie-breaking."""
    mode = case.spec.get("x")
    if mode == "ties":
        return (torch.rand(shape, generator=gen) * 3).floor()
    if mode == "equal":
        planes = torch.randint(-2, 3, shape[:3] + (1,) * (len(shape) - 3), generator=gen).float()
        return planes.expand(shape).contiguous()
    if fam == "exact":
        numel = int(torch.Size(shape).numel())
        return (torch.randperm(numel, generator=gen) - numel // 2).float().view(shape)
    return generic(gen, *shape)


def operands(case, fam):
    """CPU fp32 operands of a case from a seeded generator: ``(W or None, x [N, C, *in], M [V, N, C', *out])``."""
    gen = torch.Generator().manual_seed(zlib.crc32(case.name.encode()) + 101 * FAMILIES.index(fam))
    make = exact if fam == "exact" else generic
    W = make(gen, *weight_shape(case)) if is_conv(case.kind) else None
    x = make(gen, *in_shape(case)) if is_conv(case.kind) else _pool_input(case, fam, gen, in_shape(case))
    M = make(gen, case.spec.get("V", V_SLICES), *out_shape(case))
    return W, x, M


# ---- references (fp64, CPU) ---------------------------------------------------------------------------------------------------
def _grads(y, wrt, M):
    return torch.stack([torch.autograd.grad(y, wrt, M[v], retain_graph=True)[0] for v in range(M.shape[0])])


def maxpool_first_max(M, x, k, s, p):
    """Transposed Jacobian of a maximum pooling (floor mode, no dilation) that routes every output's cotangent to the FIRST
    element attaining the window's maximum in d-major scan order: ``M [V, N, C, OD, OH, OW]``, ``x [N, C, D, H, W]``, triples
    ``k, s, p`` -> ``[V, N, C, D, H, W]``.  Written out: pad with -inf, unfold, first index of the maximum, scatter.  The
    output extents are M's: they may be smaller than the floor formula (windows beyond them do not exist)."""
    Vd, (N, C, D, H, W) = M.shape[0], x.shape
    OD, OH, OW = M.shape[3:]
    xp = F.pad(x.to(F64), (p[2], p[2], p[1], p[1], p[0], p[0]), value=float("-inf"))
    Dp, Hp, Wp = xp.shape[2:]
    # windows that would start beyond the padded extent (an OH above the floor formula) are not a pooling's: not accepted
    assert (OD - 1) * s[0] + k[0] <= Dp and (OH - 1) * s[1] + k[1] <= Hp and (OW - 1) * s[2] + k[2] <= Wp

    def windows(t):   # [.., D', H', W'] -> [.., OD, OH, OW, kd kh kw] with the window flattened d-major
        for dim in range(3):
            t = t.unfold(2 + dim, k[dim], s[dim])
        return t[:, :, :OD, :OH, :OW].reshape(*t.shape[:2], OD, OH, OW, -1)

    win = windows(xp)
    pos = windows(torch.arange(Dp * Hp * Wp).view(1, 1, Dp, Hp, Wp))
    top = win == win.amax(-1, keepdim=True)
    first = top & (top.cumsum(-1) == 1)
    sel = (pos * first).sum(-1).reshape(1, N, C, -1).expand(Vd, N, C, -1)
    out = torch.zeros(Vd, N, C, Dp * Hp * Wp, dtype=F64)
    out.scatter_add_(3, sel, M.to(F64).reshape(Vd, N, C, -1))
    return out.view(Vd, N, C, Dp, Hp, Wp)[..., p[0]:p[0] + D, p[1]:p[1] + H, p[2]:p[2] + W].contiguous()


def _lift3(t, lead):
    """[.., L] -> [.., 1, 1, L] (``lead`` leading axes before the spatial ones)."""
    return t.reshape(*t.shape[:lead], 1, 1, t.shape[-1])


def input_rule(case, W, x, M):
    """Vector-Jacobian products of the layer for every slice of ``M``: -> ``[V, N, C, *in]`` (fp64)."""
    M = M.to(F64)
    if is_max(case.kind) and not (case.spec.get("ceil_mode") or case.spec.get("dilation", 1) != 1):
        kw = pool_kwargs(case)
        k, s, p = kw["kernel_size"], kw["stride"], kw["padding"]
        if NDIM[case.kind] == 1:
            g = maxpool_first_max(_lift3(M, 3), _lift3(x, 2), (1, 1) + k, (1, 1) + s, (0, 0) + p)
            return g.reshape(M.shape[0], *x.shape)
        return maxpool_first_max(M, x, k, s, p)
    # everything else is linear in x, or (MaxPool with ceil_mode / dilation) has distinct values and so one selection
    xi = (x.to(F64) if is_max(case.kind) else torch.zeros(x.shape, dtype=F64)).requires_grad_(True)
    y = forward(case, xi, None if W is None else W.to(F64))
    return _grads(y, xi, M)


def weight_rule(case, W, x, M):
    """Per sample and slice the vector-Jacobian product with respect to the weight: -> ``[V, N, *W.shape]`` (fp64)."""
    w = torch.zeros(W.shape, dtype=F64, requires_grad=True)
    M, x = M.to(F64), x.to(F64)
    per_n = []
    for n in range(x.shape[0]):
        y = forward(case, x[n:n + 1], w)
        per_n.append(_grads(y, w, M[:, n:n + 1]))
    return torch.stack(per_n, 1)


def n_terms(case, rule, generic_rule=False):
    """The n of the bound (n + 2) eps sum|terms| (module docstring).  ``generic_rule``: the result came from torch's own
    backward (a ``served is None`` case, or a slice the scalar kernel refused), whose order is unknown."""
    nd, s = NDIM[case.kind], case.spec
    k = tup(s["k"], nd)
    if not is_conv(case.kind):
        kd, plane = (k[0], k[1] * k[2]) if nd == 3 else (0, k[0])
        return kd + plane + (0 if is_max(case.kind) else (4 if nd == 3 else 2))
    kw = conv_kwargs(case)
    if rule == "input":
        per_launch = s["cout"] // kw["groups"] * (k[-1] if nd == 1 else k[-2] * k[-1])
        if nd < 3:
            return per_launch
        return per_launch * k[0] if generic_rule else per_launch + k[0]
    coef = tup(s["size"], nd) if is_transposed(case.kind) else out_shape(case)[2:]   # the positions of the coefficient
    if nd < 3:
        return int(torch.Size(coef).numel())
    extra = R.cdiv((k[1] - 1) * kw["dilation"][1], kw["stride"][1])
    return coef[0] * (coef[1] + extra) * coef[2]


@functools.lru_cache(maxsize=None)
def reference(name, rule, fam):
    """``(fp64 reference, sum|terms| of every entry)`` of a case, computed once per process and shared by every test that
    needs it; callers must not modify the tensors.  The bound of the generic family is ``bound(case, rule, mag)``."""
    case = ALL[name]
    W, x, M = operands(case, fam)
    fn = input_rule if rule == "input" else weight_rule
    absW = None if W is None else W.abs()
    mag = fn(case, absW, x if is_max(case.kind) else x.abs(), M.abs())
    return fn(case, W, x, M), mag


def bound(case, rule, mag, generic_rule=False):
    return (n_terms(case, rule, generic_rule) + 2) * EPS * mag


# ---- fp64 stand-ins for the four entry points ----------------------------------------------------------------------------------
Call = namedtuple("Call", "entry geom out rows")    # geom: conv_refs.Geom (pooling: Cin = Cout = planes, d = (1, 1)); out: (OH, OW)


class StandIns:
    """``kernels.conv2d_weight_mjp / conv2d_jac_t / maxpool2d_jac_t / avgpool2d_jac_t`` in torch fp64 on the CPU, signatures
    and argument checks of the wrappers, every call recorded in ``calls``.  ``install(monkeypatch)`` puts them in place."""

    def __init__(self):
        self.calls = []

    def install(self, monkeypatch):
        from vivit_amd import kernels

        for name in ("conv2d_weight_mjp", "conv2d_jac_t", "maxpool2d_jac_t", "avgpool2d_jac_t"):
            monkeypatch.setattr(kernels, name, getattr(self, name))
        return self

    @staticmethod
    def _conv_geometry(H, W, OH, OW, k, s, p, d):
        # the check of csrc/factors.hip and csrc/jacobians.hip: every output position reads inside the padded input
        assert (OH - 1) * s[0] + (k[0] - 1) * d[0] - p[0] < H + p[0] and (OW - 1) * s[1] + (k[1] - 1) * d[1] - p[1] < W + p[1], \
            f"not a convolution's geometry: image {H} x {W}, out {OH} x {OW}, k {k}, s {s}, p {p}, d {d}"

    def conv2d_weight_mjp(self, M, x, kernel_size, stride, padding, dilation):
        M, x = M.contiguous(), x.contiguous()
        Vd, N, Cout, OH, OW = M.shape
        Nx, Cin, H, W = x.shape
        if Nx != N:
            raise ValueError(f"x must have batch size {N}, got {Nx}")
        k, s, p, d = tuple(kernel_size), tuple(stride), tuple(padding), tuple(dilation)
        self._conv_geometry(H, W, OH, OW, k, s, p, d)
        self.calls.append(Call("conv2d_weight_mjp", R.Geom(Cin, Cout, H, W, k, s, p, d), (OH, OW), Vd * N))
        OHf, OWf = R.out_hw(H, W, k, s, p, d)   # >= (OH, OW) by the check above: the surplus windows are not read
        cols = F.unfold(x.to(F64), k, dilation=d, padding=p, stride=s).view(N, Cin * k[0] * k[1], OHf, OWf)[:, :, :OH, :OW]
        out = torch.einsum("vnohw,nkhw->vnok", M.to(F64), cols)
        return out.view(Vd, N, Cout, Cin, *k).to(M.dtype)

    def conv2d_jac_t(self, M, weight, in_hw, stride, padding, dilation):
        M, weight = M.contiguous(), weight.contiguous()
        Vd, N, Cout, OH, OW = M.shape
        Co, Cin, KH, KW = weight.shape
        if Co != Cout:
            raise ValueError(f"weight must have {Cout} output channels, got {Co}")
        H, W = in_hw
        k, s, p, d = (KH, KW), tuple(stride), tuple(padding), tuple(dilation)
        self._conv_geometry(H, W, OH, OW, k, s, p, d)
        self.calls.append(Call("conv2d_jac_t", R.Geom(Cin, Cout, H, W, k, s, p, d), (OH, OW), Vd * N))
        x = torch.zeros(Vd * N, Cin, H, W, dtype=F64, requires_grad=True)
        y = F.conv2d(x, weight.to(F64), None, s, p, d)[:, :, :OH, :OW]
        (g,) = torch.autograd.grad(y, x, M.to(F64).reshape(Vd * N, Cout, OH, OW))
        return g.view(Vd, N, Cin, H, W).to(M.dtype)

    def maxpool2d_jac_t(self, M, x, kernel_size, stride, padding):
        M, x = M.contiguous(), x.contiguous()
        Vd, N, C, OH, OW = M.shape
        if tuple(x.shape[:2]) != (N, C):
            raise ValueError(f"x must be [{N}, {C}, H, W], got {tuple(x.shape)}")
        H, W = x.shape[2:]
        k, s, p = tuple(kernel_size), tuple(stride), tuple(padding)
        self.calls.append(Call("maxpool2d_jac_t", R.Geom(C, C, H, W, k, s, p, (1, 1)), (OH, OW), Vd * N))
        g = maxpool_first_max(M.unsqueeze(3), x.unsqueeze(2), (1,) + k, (1,) + s, (0,) + p)
        return g.view(Vd, N, C, H, W).to(M.dtype)

    def avgpool2d_jac_t(self, M, in_hw, kernel_size, stride, padding):
        M = M.contiguous()
        Vd, N, C, OH, OW = M.shape
        H, W = in_hw
        k, s, p = tuple(kernel_size), tuple(stride), tuple(padding)
        self.calls.append(Call("avgpool2d_jac_t", R.Geom(C, C, H, W, k, s, p, (1, 1)), (OH, OW), Vd * N))
        # every window spreads its cotangent over its kh x kw positions of the padded image; crop the padding
        full = F.conv_transpose2d(M.to(F64).reshape(-1, 1, OH, OW), torch.ones(1, 1, *k, dtype=F64), stride=s)
        full = F.pad(full, (0, max(0, W + p[1] - full.shape[3]), 0, max(0, H + p[0] - full.shape[2])))
        out = full[:, :, p[0]:p[0] + H, p[1]:p[1] + W] * (1.0 / (k[0] * k[1]))
        return out.reshape(Vd, N, C, H, W).to(M.dtype)


# ---- calling the code under test ---------------------------------------------------------------------------------------------
def lower(case, rule, module, M, x):
    """The lowering function the case targets, called directly: a tensor, or ``None`` where it declines."""
    from vivit_amd.backend import extensions as ext

    kind = case.kind
    if rule == "weight":
        return (ext._hip_conv3d_weight_factor if NDIM[kind] == 3 else ext._hip_conv_weight_factor)(module, M, x)
    fn = {"conv3d": ext._hip_conv3d_jac_t, "convT3d": ext._hip_convtranspose3d_jac_t, "convT1d": ext._hip_convtranspose_jac_t,
          "convT2d": ext._hip_convtranspose_jac_t, "maxpool3d": ext._hip_pool3d_jac_t, "avgpool3d": ext._hip_pool3d_jac_t}.get(kind)
    return fn(module, M, x) if fn else ext._hip_jac_t_mat_prod(module, M, x)   # Conv1d, grouped Conv2d, pooling in one dimension


def dispatch(case, rule, module, M, x):
    """The same through the dispatch: ``_param_factor`` / ``_jac_t_mat_prod``."""
    from vivit_amd.backend import extensions as ext

    return ext._param_factor(module, "weight", M, x) if rule == "weight" else ext._jac_t_mat_prod(module, M, x)


def on_device(case, fam, device, dtype=torch.float32):
    """``(module, x, M)`` of a case on ``device``."""
    W, x, M = operands(case, fam)
    return make_module(case, W).to(device=device, dtype=dtype), x.to(device=device, dtype=dtype), M.to(device=device, dtype=dtype)


def routes(calls):
    """The planner route of every recorded convolution call, by the mirrors of tests/conv_refs.py on the 2-D geometry the
    lowering handed over: the set of (entry, route)."""
    got = set()
    for c in calls:
        if c.entry == "conv2d_weight_mjp":
            got.add(("weight", R.weight_plan(c.geom, out=c.out)["route"]))
        elif c.entry == "conv2d_jac_t":
            got.add(("input", R.input_plan(c.geom, rows=c.rows, out=c.out)["route"]))
    return got


# ---- the cases ---------------------------------------------------------------------------------------------------------------
# expects: lowering (the function the case is there for), edge (what it exercises), served ("hip": the lowering returns a
# tensor; None: it declines and the generic rule serves the layer) with reason, input_route / weight_route (the planner route of
# the per-tap 2-D geometry; None where no launch happens), zero_depth (input depth slices no window reaches), families.
def conv(name, kind, cin, cout, k, size, *, lowering, edge, input_route="scalar", weight_route="scalar", served="hip", reason=None,
         zero_depth=(), **geometry):
    spec = dict(cin=cin, cout=cout, k=k, size=size, **geometry)
    return Case(name, kind, spec, dict(lowering=lowering, edge=edge, served=served, reason=reason, input_route=input_route,
                                       weight_route=weight_route, zero_depth=tuple(zero_depth)))


def pool(name, kind, c, k, size, *, lowering, edge, served="hip", reason=None, zero_depth=(), families=FAMILIES, **geometry):
    spec = dict(c=c, k=k, size=size, **geometry)
    return Case(name, kind, spec, dict(lowering=lowering, edge=edge, served=served, reason=reason, zero_depth=tuple(zero_depth),
                                       families=tuple(families)))


C3 = "_hip_conv3d_jac_t / _conv3d_weight_contract"
T2 = "_convtranspose2d_input / _hip_conv_weight_factor"
T3 = "_hip_convtranspose3d_jac_t / _hip_conv3d_weight_factor"
J2 = "_hip_jac_t_mat_prod / _hip_conv_weight_factor"
P3 = "_hip_pool3d_jac_t"

CONV3D_CASES = [
    conv("c3-empty-tap", "conv3d", 2, 3, (3, 2, 2), (2, 4, 4), s=(3, 1, 1), p=(2, 0, 0), lowering=C3,
         edge="D = 2, KD = 3, pd = 2, sd = 3: tap 1 has no partner at all (_depth_range empty), taps 0 and 2 a single slice"),
    conv("c3-single-slice", "conv3d", 2, 3, (2, 2, 2), (3, 4, 3), s=(2, 1, 1), p=(1, 0, 0), lowering=C3,
         edge="tap 0 reaches one slice (q_lo = q_hi = 1), tap 1 two"),
    conv("c3-od1", "conv3d", 3, 2, (3, 2, 2), (3, 4, 5), lowering=C3, edge="OD = 1: the batch of 2-D problems is N"),
    conv("c3-cross-slice", "conv3d", 2, 3, (2, 3, 2), (3, 6, 5), d=(1, 2, 1), lowering=C3,
         edge="(KH - 1) dh = 4 > sh = 1: four zero rows behind every coefficient slice, windows run into the next slice"),
    conv("c3-unread-rows", "conv3d", 2, 3, (2, 1, 2), (3, 8, 4), s=(1, 3, 1), lowering=C3,
         edge="KH = 1, sh = 3, H = 8: image row 7 lies in no window"),
    conv("c3-bigpad", "conv3d", 2, 3, 2, (2, 3, 3), p=(2, 3, 3), lowering=C3,
         edge="padding 2 and 3 against a kernel extent of 1: whole taps and windows in the padding"),
    conv("c3-asym", "conv3d", 3, 5, (3, 2, 3), (6, 7, 5), s=(2, 1, 3), p=(1, 0, 2), d=(1, 2, 1), lowering=C3,
         edge="stride, padding and dilation differ on every axis"),
    conv("c3-kd1-sd2", "conv3d", 2, 3, (1, 2, 2), (5, 4, 4), s=(2, 1, 1), zero_depth=(1, 3), lowering=C3,
         edge="KD = 1, sd = 2: input slices 1 and 3 receive nothing"),
    conv("c3-g2", "conv3d", 4, 6, (2, 3, 2), (4, 5, 4), g=2, p=(1, 1, 0), lowering=C3, edge="groups 2, Cout/G = 3, Cin/G = 2"),
    conv("c3-g3", "conv3d", 3, 6, 2, (3, 4, 4), g=3, s=(1, 2, 1), lowering=C3, edge="groups 3, Cout/G = 2, Cin/G = 1"),
    conv("c3-w-mfma", "conv3d", 8, 32, 3, (4, 8, 8), p=1, weight_route="mfma", lowering=C3,
         edge="the stack (42 x 8 image, two zero rows per slice, padding (0, 1)) on the weight rule's matrix pipe"),
    conv("c3-w-lds", "conv3d", 16, 4, 3, (8, 16, 16), p=1, lowering=C3,
         edge="the stack (146 x 16 image of 16 channels) is refused LDS and falls to the scalar weight kernel"),
    conv("c3-in-mfma", "conv3d", 4, 128, (2, 3, 3), (3, 5, 5), input_route="mfma", lowering=C3,
         edge="Cout KH KW = 1152 > 1024: the input rule's matrix pipe with batch N OD"),
    conv("c3-in-mfma-g2", "conv3d", 4, 256, (2, 3, 3), (3, 5, 5), g=2, input_route="mfma", lowering=C3,
         edge="the same grouped: 1152 filter elements per group, Cin/G = 2"),
]

CONVT_CASES = [
    conv("t1-op-dil2", "convT1d", 2, 3, 2, 5, d=2, op=1, lowering=T2, edge="output_padding 1 with stride 1, dilation 2: OW < floor formula"),
    conv("t2-op-dil2", "convT2d", 2, 3, 2, (3, 4), d=2, op=1, lowering=T2,
         edge="output_padding 1 with stride 1, dilation 2: the image is wider and taller than the windows reach"),
    conv("t3-op-dil2", "convT3d", 2, 3, 2, (2, 3, 3), d=2, op=1, lowering=T3, edge="the same in three dimensions"),
    conv("t1-s3-k2", "convT1d", 3, 2, 2, 4, s=3, lowering=T2, edge="stride 3, kernel 2: two of three output columns per step carry a tap"),
    conv("t2-s3-k2", "convT2d", 3, 2, 2, (3, 2), s=3, op=(2, 0), lowering=T2, edge="stride 3, kernel 2, output_padding (2, 0)"),
    conv("t3-s3-k2", "convT3d", 3, 2, 2, (2, 2, 3), s=3, op=(1, 0, 2), lowering=T3, edge="stride 3, kernel 2, output_padding (1, 0, 2)"),
    conv("t1-g2", "convT1d", 4, 6, 3, 4, g=2, s=2, p=1, lowering=T2, edge="groups 2, Cin/G = 2, Cout/G = 3"),
    conv("t2-g2", "convT2d", 4, 6, (3, 2), (3, 4), g=2, s=(2, 1), p=(1, 0), lowering=T2, edge="groups 2, Cin/G = 2, Cout/G = 3"),
    conv("t3-g2", "convT3d", 4, 6, (2, 3, 2), (2, 3, 3), g=2, s=(1, 2, 1), p=(0, 1, 0), lowering=T3, edge="groups 2, Cin/G = 2, Cout/G = 3"),
    conv("t1-hq1", "convT1d", 2, 3, 3, 1, s=2, lowering=T2, edge="a single input position"),
    conv("t2-hq1", "convT2d", 2, 3, 3, (1, 1), s=2, op=1, lowering=T2, edge="a single input position (hq = (1, 1))"),
    conv("t3-hq1", "convT3d", 2, 3, (2, 3, 2), (1, 1, 1), s=2, lowering=T3, edge="a single input position"),
    conv("t3-asym", "convT3d", 3, 5, (2, 3, 3), (3, 4, 3), s=(3, 1, 2), p=(1, 2, 0), d=(1, 1, 2), op=(2, 0, 1), lowering=T3,
         edge="stride, padding, dilation and output_padding differ on every axis; depth taps with one partner"),
    conv("t3-hrows", "convT3d", 2, 2, 2, (2, 3, 3), d=3, op=2, lowering=T3,
         edge="output_padding 2 >= stride + padding: hrows < H, the image's last rows lie beyond the slice pitch"),
    conv("t2-p-beyond", "convT2d", 2, 3, 2, (4, 4), s=2, p=2, served=None, reason="p > (K - 1) d", input_route=None, lowering=T2,
         edge="padding 2 > (K - 1) d = 1: the reversed rule would need negative padding"),
    conv("t3-p-beyond", "convT3d", 2, 3, 2, (3, 4, 4), s=2, p=(0, 2, 0), served=None, reason="p > (K - 1) d", input_route=None, lowering=T3,
         edge="the same on the height axis of a 3-D layer"),
    conv("t1-wide", "convT1d", 2, 600, 2, 3, served=None, reason="Cout/G kh kw > 1024", input_route=None, lowering=T2,
         edge="1200 filter elements: declined although the matrix-pipe input kernel serves such slices (pins today's behaviour)"),
    conv("t2-wide", "convT2d", 2, 130, 3, (2, 2), served=None, reason="Cout/G kh kw > 1024", input_route=None, lowering=T2,
         edge="1170 filter elements: declined likewise"),
    conv("t2-w-mfma", "convT2d", 16, 8, 3, (8, 8), p=1, weight_route="mfma", lowering=T2,
         edge="weight rule with V N rows behind a leading V = 1 (the slice axis folded into the batch) on the matrix pipe"),
    conv("t3-w-mfma", "convT3d", 8, 8, 3, (3, 6, 6), p=1, weight_route="mfma", lowering=T3,
         edge="the same through the stack of the 3-D rule"),
]

ROW_CASES = [
    conv("c1-len1", "conv1d", 2, 3, 3, 1, p=1, lowering=J2, edge="length 1: a 1 x 1 image, two of three taps in the padding"),
    conv("c1-stride-beyond", "conv1d", 2, 3, 2, 8, s=3, lowering=J2, edge="stride 3 beyond kernel 2: every third column receives nothing"),
    conv("c1-g3", "conv1d", 3, 6, 3, 7, g=3, p=1, d=2, lowering=J2, edge="groups 3, Cout/G = 2, Cin/G = 1"),
    conv("c2-g3", "conv2d", 6, 3, (3, 2), (5, 6), g=3, s=(1, 2), p=(1, 0), lowering=J2, edge="groups 3, Cout/G = 1, Cin/G = 2"),
    conv("c2-g2-stride-beyond", "conv2d", 4, 6, 2, (7, 7), g=2, s=3, lowering=J2, edge="groups 2 with stride 3 beyond kernel 2"),
    pool("a1-pad", "avgpool1d", 3, 4, 7, s=3, p=2, lowering="_hip_jac_t_mat_prod", edge="AvgPool1d with padding, window 4 (a power of two)"),
    pool("a1-pad-k3", "avgpool1d", 3, 3, 7, s=2, p=1, families=("generic",), lowering="_hip_jac_t_mat_prod",
         edge="AvgPool1d with padding, window 3: the reciprocal is rounded"),
    pool("a1-len1", "avgpool1d", 2, 1, 1, lowering="_hip_jac_t_mat_prod", edge="length 1"),
    pool("m1-ties", "maxpool1d", 3, 3, 9, s=2, p=1, x="ties", lowering="_hip_jac_t_mat_prod", edge="MaxPool1d with tied maxima: the first wins"),
    pool("m1-len1", "maxpool1d", 2, 1, 1, lowering="_hip_jac_t_mat_prod", edge="length 1"),
]

POOL3D_CASES = [
    pool("m3-kd11", "maxpool3d", 2, (2, 1, 1), (5, 3, 4), lowering=P3, edge="(kd, 1, 1) window: only the depth stage selects"),
    pool("m3-1hw", "maxpool3d", 2, (1, 2, 3), (3, 5, 7), s=(1, 2, 2), lowering=P3, edge="(1, kh, kw) window: only the plane stage selects"),
    pool("m3-pad-depth", "maxpool3d", 2, 2, (5, 4, 4), p=(1, 0, 0), lowering=P3, edge="padding on the depth axis only"),
    pool("m3-stride-beyond", "maxpool3d", 2, 2, (6, 4, 5), s=(3, 2, 2), zero_depth=(2, 5), lowering=P3,
         edge="depth stride 3 beyond kernel 2: slices 2 and 5 are read by no window"),
    pool("m3-ties", "maxpool3d", 3, (3, 2, 2), (6, 7, 5), s=(1, 2, 1), p=(1, 1, 0), x="ties", lowering=P3,
         edge="floor(3 rand): many tied maxima, overlapping windows; first maximum in d-major order"),
    pool("m3-equal-planes", "maxpool3d", 2, (2, 3, 2), (4, 5, 4), s=(1, 2, 2), p=(1, 1, 1), x="equal", lowering=P3,
         edge="every plane constant: the plane stage ties everywhere, the depth stage decides"),
    pool("a3-kd11", "avgpool3d", 2, (2, 1, 1), (5, 3, 4), lowering=P3, edge="(kd, 1, 1) window"),
    pool("a3-1hw", "avgpool3d", 2, (1, 2, 2), (3, 5, 6), s=(1, 2, 1), lowering=P3, edge="(1, kh, kw) window"),
    pool("a3-pad-depth", "avgpool3d", 2, 2, (5, 4, 4), p=(1, 0, 0), lowering=P3, edge="padding on the depth axis only"),
    pool("a3-stride-beyond", "avgpool3d", 2, 2, (6, 4, 5), s=(3, 2, 2), zero_depth=(2, 5), lowering=P3,
         edge="depth stride 3 beyond kernel 2: slices 2 and 5 are read by no window"),
    pool("a3-k323", "avgpool3d", 2, (3, 2, 3), (6, 5, 7), s=(2, 1, 2), p=(1, 1, 1), families=("generic",), lowering=P3,
         edge="window 3 x (2 x 3): both reciprocals are rounded"),
    pool("m3-ceil", "maxpool3d", 2, 2, (5, 5, 5), ceil_mode=True, served=None, reason="ceil_mode", lowering=P3, edge="declined: ceil_mode"),
    pool("m3-dilation", "maxpool3d", 2, 2, (5, 5, 5), dilation=2, served=None, reason="dilation", lowering=P3, edge="declined: dilation"),
    pool("a3-ceil", "avgpool3d", 2, 2, (5, 5, 5), ceil_mode=True, served=None, reason="ceil_mode", lowering=P3, edge="declined: ceil_mode"),
    pool("a3-no-pad-count", "avgpool3d", 2, 2, (4, 4, 4), p=1, count_include_pad=False, served=None, reason="count_include_pad=False",
         lowering=P3, edge="declined: count_include_pad=False"),
    pool("a3-divisor", "avgpool3d", 2, 2, (4, 4, 4), divisor_override=4, served=None, reason="divisor_override", lowering=P3,
         edge="declined: divisor_override"),
]

CASES = CONV3D_CASES + CONVT_CASES + ROW_CASES + POOL3D_CASES
NAMES = [c.name for c in CASES]
ALL = {c.name: c for c in CASES}
assert len(ALL) == len(CASES)
RUNS = [(c.name, rule, fam) for c in CASES for rule in rules_of(c) for fam in families_of(c)]   # every (case, rule, family)
MFMA_RUNS = [(n, r, f) for n, r, f in RUNS if ALL[n].expects.get(r + "_route") == "mfma"]


def declines(case):
    """Whether the input lowering of a transposed case declines (returns ``None``): ``p > (K - 1) d`` on one of the axes
    ``_convtranspose2d_input`` sees (height and width; a 1-D layer's only axis), or more than 1024 filter elements per launch.
    The depth axis has neither limit -- and a 3-D layer none of whose depth taps has a partner never reaches the 2-D rule: its
    Jacobian is zero and the lowering says so."""
    nd, kw = NDIM[case.kind], conv_kwargs(case)
    k, s, p, d = tup(case.spec["k"], nd), kw["stride"], kw["padding"], kw["dilation"]
    if nd == 3:
        QD, Dm = case.spec["size"][0], out_shape(case)[2]
        if not any(0 <= q * s[0] - p[0] + kd * d[0] < Dm for q in range(QD) for kd in range(k[0])):
            return False
    hw = slice(-2, None)
    filt = case.spec["cout"] // kw["groups"] * int(torch.Size(k[hw]).numel())
    return any(p_ > (k_ - 1) * d_ for k_, p_, d_ in zip(k[hw], p[hw], d[hw])) or filt > 1024
