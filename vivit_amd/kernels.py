"""Host-side launchers: torch tensors in, HIP kernels (libvivit_hip.so) out.

PyTorch is plumbing here (device memory, streams); all arithmetic happens in the hand-written
gfx950 kernels behind the C ABI of ``include/vivit_hip.h``.  Every function raises
``RuntimeError`` for tensors that are not fp32 HIP-device tensors: there is deliberately no CPU
path and no backend switch (host-logic tests monkeypatch these functions from ``tests/helpers.py``).
"""
import ctypes
import functools
import math
from typing import Optional, Tuple

import torch

from vivit_amd import _lib

_WORKSPACES = {}


def _require_device(*tensors):
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "vivit_amd kernels need HIP-device tensors (got a CPU tensor); there is no CPU fallback"
            )
        if t.dtype != torch.float32:
            raise RuntimeError(f"vivit_amd kernels are fp32 only (got {t.dtype})")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"all operands must live on one device (got {dev} and {t.device})")


def _first_device(args, kwargs):
    for a in list(args) + list(kwargs.values()):
        if isinstance(a, torch.Tensor):
            return a.device if a.is_cuda else None
        if isinstance(a, (list, tuple)) and a and isinstance(a[0], torch.Tensor):
            return a[0].device if a[0].is_cuda else None
    return None


def _launcher(fn):
    """Run ``fn`` with the HIP device of its first tensor operand current.

    The C side launches on the *current* device (``<<<>>>`` on the given stream, the dynamic-LDS attribute bitmap is
    keyed on ``hipGetDevice``), so a process that drives several GPUs must switch before every call -- torch ops do
    that implicitly, a raw ctypes call does not."""

    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        dev = _first_device(args, kwargs)
        if dev is None or dev.index == torch.cuda.current_device():
            return fn(*args, **kwargs)
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)

    return wrapped


def _launcher_method(fn):
    """``_launcher`` for methods whose device is that of ``self.evals``."""

    @functools.wraps(fn)
    def wrapped(self, *args, **kwargs):
        dev = self.evals.device
        if not dev.type == "cuda" or dev.index == torch.cuda.current_device():
            return fn(self, *args, **kwargs)
        with torch.cuda.device(dev):
            return fn(self, *args, **kwargs)

    return wrapped


def _check_out(out, m, n, *operands):
    """``out`` is written by the kernel with a single leading dimension: shape, strides and aliasing must be right,
    otherwise the launch would write out of bounds or into an operand it is still reading."""
    if out is None:
        return
    if tuple(out.shape) != (m, n):
        raise ValueError(f"out must have shape {(m, n)}, got {tuple(out.shape)}")
    if out.numel() > 0 and (out.stride(1) != 1 or (m > 1 and out.stride(0) < n)):
        raise ValueError(f"out must be row-major with unit column stride (strides {out.stride()})")
    for t in operands:
        if t is not None and t.numel() > 0 and out.numel() > 0 and t.untyped_storage().data_ptr() == out.untyped_storage().data_ptr():
            lo, hi = out.data_ptr(), out.data_ptr() + 4 * ((m - 1) * out.stride(0) + n)
            tlo = t.data_ptr()
            thi = tlo + 4 * (sum((sz - 1) * st for sz, st in zip(t.shape, t.stride())) + 1)
            if tlo < hi and lo < thi:
                raise ValueError("out must not alias an input operand")


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _workspace(nbytes: int, like: torch.Tensor):
    """Stream-ordered scratch buffer (grown on demand, cached per device and stream)."""
    if nbytes == 0:
        return None, 0
    key = (like.device, _stream(like))
    buf = _WORKSPACES.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = None
        # The old buffer is released BEFORE the larger one is allocated, so the two never coexist (a caller that bounds its peak
        # memory, _linear_seq_weight_closures, counts one scratch buffer).  Safe: the key is the launch stream, every kernel that
        # used the old buffer was enqueued on it, and torch's allocator hands a freed block out again in that stream's order only.
        _WORKSPACES.pop(key, None)
        buf = torch.empty(_workspace_alloc_bytes(nbytes), dtype=torch.uint8, device=like.device)
        _WORKSPACES[key] = buf
    return buf.data_ptr(), buf.numel()


def _as2d(t: torch.Tensor) -> torch.Tensor:
    if t.dim() != 2:
        raise ValueError(f"expected a matrix, got {t.dim()} dimensions")
    if t.numel() > 0 and t.stride(1) != 1:
        t = t.contiguous()
    if t.numel() > 0 and t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t


def _ld(t):
    return max(t.stride(0), t.shape[1], 1) if t.shape[0] > 1 else max(t.shape[1], 1)


def _workspace_alloc_bytes(nbytes: int) -> int:
    """What :func:`_workspace` allocates for a request of ``nbytes``."""
    return int(nbytes * 1.25) + 256 if nbytes else 0


def gram_syrk_workspace_bytes(n: int, p: int) -> int:
    """Bytes of the scratch buffer ``gram_syrk`` takes for ``A: [n, p]`` (a host-side query: no device is touched)."""
    return _workspace_alloc_bytes(_lib.load().vivit_gram_syrk_f32_workspace_bytes(n, p))


def gemm_workspace_bytes(m: int, n: int, k: int) -> int:
    """Bytes of the scratch buffer ``gemm_nt`` / ``gemm_nn`` / ``gemm_tn`` take for an ``[m, n]`` output with contraction ``k``."""
    return _workspace_alloc_bytes(_lib.load().vivit_gemm_f32_workspace_bytes(m, n, k))


@_launcher
def gram_syrk(A: torch.Tensor, out: Optional[torch.Tensor] = None, alpha: float = 1.0, beta: float = 0.0):
    """``out = alpha * A @ A.T + beta * out`` for ``A: [n, p]`` (K1, MFMA SYRK)."""
    _require_device(A, out)
    A = _as2d(A)
    n, p = A.shape
    _check_out(out, n, n, A)
    if out is None:
        out = torch.empty((n, n), dtype=torch.float32, device=A.device)
        beta = 0.0
    lib = _lib.load()
    ws, wsb = _workspace(lib.vivit_gram_syrk_f32_workspace_bytes(n, p), A)
    st = lib.vivit_gram_syrk_f32(A.data_ptr(), n, p, _ld(A), out.data_ptr(), _ld(out), alpha, beta, ws, wsb, _stream(A))
    _lib.check(st, "vivit_gram_syrk_f32")
    return out


def _gemm(name, A, B, m, n, k, out, alpha, beta):
    lib = _lib.load()
    _check_out(out, m, n, A, B)
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=A.device)
        beta = 0.0
    ws, wsb = _workspace(lib.vivit_gemm_f32_workspace_bytes(m, n, k), A)
    st = getattr(lib, name)(
        A.data_ptr(), B.data_ptr(), out.data_ptr(), m, n, k, _ld(A), _ld(B), _ld(out), alpha, beta, ws, wsb, _stream(A)
    )
    _lib.check(st, name)
    return out


@_launcher
def gemm_nt(A, B, out=None, alpha: float = 1.0, beta: float = 0.0):
    """``out = alpha * A @ B.T + beta * out``; ``A: [m, k]``, ``B: [n, k]`` (K2/K9)."""
    _require_device(A, B, out)
    A, B = _as2d(A), _as2d(B)
    if A.shape[1] != B.shape[1]:
        raise ValueError("Trailing dimensions don't match.")
    return _gemm("vivit_gemm_nt_f32", A, B, A.shape[0], B.shape[0], A.shape[1], out, alpha, beta)


@_launcher
def gemm_nn(A, B, out=None, alpha: float = 1.0, beta: float = 0.0):
    """``out = alpha * A @ B + beta * out``; ``A: [m, k]``, ``B: [k, n]`` (K6/K7/K8)."""
    _require_device(A, B, out)
    A, B = _as2d(A), _as2d(B)
    if A.shape[1] != B.shape[0]:
        raise ValueError("Inner dimensions don't match.")
    return _gemm("vivit_gemm_nn_f32", A, B, A.shape[0], B.shape[1], A.shape[1], out, alpha, beta)


@_launcher
def gemm_tn(A, B, out=None, alpha: float = 1.0, beta: float = 0.0):
    """``out = alpha * A.T @ B + beta * out``; ``A: [k, m]``, ``B: [k, n]`` (K5)."""
    _require_device(A, B, out)
    A, B = _as2d(A), _as2d(B)
    if A.shape[0] != B.shape[0]:
        raise ValueError("Leading dimensions don't match.")
    return _gemm("vivit_gemm_tn_f32", A, B, A.shape[1], B.shape[1], A.shape[0], out, alpha, beta)


@_launcher
def gram_hadamard(Gz, Gs, C: int, N: int, out=None, alpha: float = 1.0, beta: float = 0.0):
    """``out[c,n,d,m] = alpha * Gz[n,m] * Gs[c,n,d,m] + beta * out`` (K1')."""
    _require_device(Gz, Gs, out)
    Gz, Gs = Gz.contiguous(), Gs.contiguous()
    if out is None:
        out = torch.empty((C * N, C * N), dtype=torch.float32, device=Gz.device)
        beta = 0.0
    if not out.is_contiguous() or tuple(out.shape) != (C * N, C * N):
        raise ValueError(f"out must be a contiguous [{C * N}, {C * N}] matrix")
    if tuple(Gz.shape) != (N, N) or Gs.numel() != (C * N) ** 2:
        raise ValueError("Gz must be [N, N] and Gs [C*N, C*N]")
    st = _lib.load().vivit_gram_hadamard_f32(Gz.data_ptr(), Gs.data_ptr(), out.data_ptr(), C, N, alpha, beta, _stream(Gz))
    _lib.check(st, "vivit_gram_hadamard_f32")
    return out


@_launcher
def gram_hadamard_block(Gz, Gs, Cr: int, Nr: int, Cc: int, Nc: int, out=None, alpha: float = 1.0, beta: float = 0.0):
    """``out[(c,n),(d,m)] = alpha * Gz[n,m] * Gs[(c,n),(d,m)] + beta * out`` for a rectangular block (rows
    ``Cr x Nr``, columns ``Cc x Nc``): the block row of a batch shard, and ``V^T g`` of a factorised Linear weight."""
    _require_device(Gz, Gs, out)
    Gz, Gs = Gz.contiguous(), Gs.contiguous()
    rows, cols = Cr * Nr, Cc * Nc
    if tuple(Gz.shape) != (Nr, Nc) or Gs.numel() != rows * cols:
        raise ValueError(f"Gz must be [{Nr}, {Nc}] and Gs [{rows}, {cols}]")
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.float32, device=Gz.device)
        beta = 0.0
    _check_out(out, rows, cols, Gz, Gs)
    st = _lib.load().vivit_gram_hadamard_block_f32(Gz.data_ptr(), Gs.data_ptr(), out.data_ptr(), Cr, Nr, Cc, Nc, _ld(out),
                                                   alpha, beta, _stream(Gz))
    _lib.check(st, "vivit_gram_hadamard_block_f32")
    return out


@_launcher
def gram_seq_reduce(Gz, Gs, Cr: int, Nr: int, Cc: int, Nc: int, T: int, out=None, alpha: float = 1.0, beta: float = 0.0):
    """``out[(c,n),(e,m)] = alpha * sum_{t,u<T} Gz[(n,t),(m,u)] * Gs[(c,n,t),(e,m,u)] + beta * out`` for a rectangular block (rows
    ``Cr x Nr``, columns ``Cc x Nc``): the Gram matrix of a Linear weight on a sequence input from the Gram matrices of its two
    factors.  ``Gz [Nr T, Nc T]``, ``Gs [Cr Nr T, Cc Nc T]`` and ``out [Cr Nr, Cc Nc]`` may be row-strided views."""
    _require_device(Gz, Gs, out)
    Gz, Gs = _as2d(Gz), _as2d(Gs)
    rows, cols = Cr * Nr, Cc * Nc
    if tuple(Gz.shape) != (Nr * T, Nc * T) or tuple(Gs.shape) != (rows * T, cols * T):
        raise ValueError(f"Gz must be [{Nr * T}, {Nc * T}] and Gs [{rows * T}, {cols * T}], got {tuple(Gz.shape)} and {tuple(Gs.shape)}")
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.float32, device=Gz.device)
        beta = 0.0
    _check_out(out, rows, cols, Gz, Gs)
    st = _lib.load().vivit_gram_seq_reduce_f32(Gz.data_ptr(), _ld(Gz), Gs.data_ptr(), _ld(Gs), out.data_ptr(), _ld(out), Cr, Nr, Cc, Nc,
                                               T, alpha, beta, _stream(Gz))
    _lib.check(st, "vivit_gram_seq_reduce_f32")
    return out


@_launcher
def symmetrize_lower(G):
    """``G[i, j] = G[j, i]`` for ``j > i``, in place, for a square row-strided ``G``; returns ``G``."""
    _require_device(G)
    n = G.shape[0]
    if G.dim() != 2 or G.shape[1] != n or (G.numel() > 0 and (G.stride(1) != 1 or (n > 1 and G.stride(0) < n))):
        raise ValueError("G must be a square row-major matrix with unit column stride")
    _lib.check(_lib.load().vivit_symmetrize_lower_f32(G.data_ptr(), n, _ld(G), _stream(G)), "vivit_symmetrize_lower_f32")
    return G


@_launcher
def class_contract(mat, s):
    """``T[f,o,n] = sum_c mat[f,c,n] s[c,n,o]``; ``mat: [F,C,N]``, ``s: [C,N,O]`` (first half of linear.py:53)."""
    _require_device(mat, s)
    mat, s = mat.contiguous(), s.contiguous()
    F, C, N = mat.shape
    if tuple(s.shape[:2]) != (C, N):
        raise ValueError(f"s must be [{C}, {N}, O], got {tuple(s.shape)}")
    O = s.shape[2]
    T = torch.empty((F, O, N), dtype=torch.float32, device=mat.device)
    st = _lib.load().vivit_class_contract_f32(mat.data_ptr(), s.data_ptr(), T.data_ptr(), F, C, N, O, _stream(mat))
    _lib.check(st, "vivit_class_contract_f32")
    return T


@_launcher
def class_expand(s, U):
    """``R[f,c,n] = sum_o s[c,n,o] U[f,o,n]``; ``s: [C,N,O]``, ``U: [F,O,N]`` (second half of linear.py:64)."""
    _require_device(s, U)
    s, U = s.contiguous(), U.contiguous()
    C, N, O = s.shape
    F = U.shape[0]
    if tuple(U.shape[1:]) != (O, N):
        raise ValueError(f"U must be [F, {O}, {N}], got {tuple(U.shape)}")
    R = torch.empty((F, C, N), dtype=torch.float32, device=s.device)
    st = _lib.load().vivit_class_expand_f32(s.data_ptr(), U.data_ptr(), R.data_ptr(), F, C, N, O, _stream(s))
    _lib.check(st, "vivit_class_expand_f32")
    return R


@_launcher
def symeig(G: torch.Tensor, eigenvectors: bool = False, overwrite: bool = False, info_out: Optional[list] = None
           ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Eigenvalues (ascending) and, optionally, column eigenvectors of symmetric ``G`` (K3/K4).

    Raises ``RuntimeError`` if the solver reports unconverged eigenvalues (the reference's
    behaviour for a failing ``Tensor.symeig``, vivit/utils/eig.py:37-40).  That check reads the device-side
    ``info`` word, i.e. synchronises with the stream; a caller that wants to stay asynchronous passes a list as
    ``info_out``: the ``info`` tensor is appended to it instead and nothing is read back (check it with
    :func:`check_info` when convenient).
    """
    _require_device(G)
    if G.dim() != 2 or G.shape[0] != G.shape[1]:
        raise ValueError(f"Input must be a square matrix. Got shape {tuple(G.shape)}.")
    n = G.shape[0]
    lib = _lib.load()

    def solve():
        A = _as2d(G)
        if A.data_ptr() == G.data_ptr() and not overwrite:
            A = A.clone()  # the solver destroys its input (reflectors are stored in it)
        w = torch.empty(n, dtype=torch.float32, device=G.device)
        Z = torch.empty((n, n), dtype=torch.float32, device=G.device) if eigenvectors else None
        info = torch.zeros(1, dtype=torch.int32, device=G.device)
        ws, wsb = _workspace(lib.vivit_symeig_f32_workspace_bytes(n, 1 if eigenvectors else 0), G)
        st = lib.vivit_symeig_f32(
            A.data_ptr(), n, _ld(A), w.data_ptr(), Z.data_ptr() if eigenvectors else None, n, ws, wsb, info.data_ptr(), _stream(G)
        )
        _lib.check(st, "vivit_symeig_f32")
        if info_out is not None:
            info_out.append(info)
        else:
            check_info(info)  # device->host sync; the reference syncs here too (criterion callback)
        return w, Z

    return _retry_on_launch_chain(solve, intact=not overwrite, G=G)


@_launcher
def linear_weight_mjp(s, z):
    """``V_t[c,n,o,i] = s[c,n,o] z[n,i]`` materialised (``param_mjp`` of a Linear weight, einsum "vno,ni->vnoi")."""
    _require_device(s, z)
    s, z = s.contiguous(), z.contiguous()
    C, N, O = s.shape
    if z.shape[0] != N:
        raise ValueError(f"z must be [{N}, in], got {tuple(z.shape)}")
    I = z.shape[1]
    V = torch.empty((C, N, O, I), dtype=torch.float32, device=s.device)
    st = _lib.load().vivit_linear_weight_mjp_f32(s.data_ptr(), z.data_ptr(), V.data_ptr(), C, N, O, I, _stream(s))
    _lib.check(st, "vivit_linear_weight_mjp_f32")
    return V


@_launcher
def conv2d_weight_mjp(M, x, kernel_size, stride, padding, dilation):
    """``param_mjp`` of a Conv2d weight (groups = 1, zero padding): ``M [V, N, Cout, OH, OW]``, ``x [N, Cin, H, W]`` ->
    ``[V, N, Cout, Cin, KH, KW]`` (unfold + einsum "vnol,nkl->vnok" without the im2col buffer)."""
    _require_device(M, x)
    M, x = M.contiguous(), x.contiguous()
    Vd, N, Cout, OH, OW = M.shape
    Nx, Cin, H, W = x.shape
    if Nx != N:
        raise ValueError(f"x must have batch size {N}, got {Nx}")
    KH, KW = kernel_size
    out = torch.empty((Vd, N, Cout, Cin, KH, KW), dtype=torch.float32, device=M.device)
    st = _lib.load().vivit_conv2d_weight_mjp_f32(
        M.data_ptr(), x.data_ptr(), out.data_ptr(), Vd * N, N, Cin, H, W, Cout, KH, KW, OH, OW, stride[0], stride[1],
        padding[0], padding[1], dilation[0], dilation[1], _stream(M))
    _lib.check(st, "vivit_conv2d_weight_mjp_f32")
    return out


ACTIVATION_KINDS = {"relu": 0, "sigmoid": 1, "tanh": 2, "leaky_relu": 3, "logsigmoid": 4, "elu": 5, "selu": 6, "gelu": 7,
                    "gelu_tanh": 8, "silu": 9, "softcap": 10}


@_launcher
def act_jac_t(M, x, kind: str, param: float = 0.0):
    """``out[v, n, ...] = M[v, n, ...] * f'(x[n, ...])`` for an elementwise activation ``f`` (``kind`` in
    :data:`ACTIVATION_KINDS`): the transposed input-Jacobian of SqrtGGN{ReLU,Sigmoid,Tanh,...} and of GELU (``"gelu"``: erf form,
    ``"gelu_tanh"``: ``approximate='tanh'``) and SiLU.  ``"softcap"``: ``f(x) = param * tanh(x / param)`` with the cap ``param``, a
    finite float ``> 0`` (Gemma-2's final logits)."""
    if kind == "softcap":
        param = _softcap(param)
    _require_device(M, x)
    M, x = M.contiguous(), x.contiguous()
    if tuple(M.shape[1:]) != tuple(x.shape):
        raise ValueError(f"M must be [V, *x.shape], got {tuple(M.shape)} for x {tuple(x.shape)}")
    out = torch.empty_like(M)
    st = _lib.load().vivit_act_jac_t_f32(M.data_ptr(), x.data_ptr(), out.data_ptr(), M.shape[0], x.numel(), ACTIVATION_KINDS[kind],
                                        float(param), _stream(M))
    _lib.check(st, "vivit_act_jac_t_f32")
    return out


@_launcher
def channel_scale(M, scale):
    """``out[v, n, c, ...] = M[v, n, c, ...] * scale[c]`` (BatchNorm in eval mode)."""
    _require_device(M, scale)
    M, scale = M.contiguous(), scale.contiguous()
    C = scale.numel()
    if M.dim() < 3 or M.shape[2] != C:
        raise ValueError(f"M must be [V, N, {C}, ...], got {tuple(M.shape)}")
    L = M[0, 0, 0].numel()
    out = torch.empty_like(M)
    st = _lib.load().vivit_channel_scale_f32(M.data_ptr(), scale.data_ptr(), out.data_ptr(), M.shape[0] * M.shape[1], C, L, _stream(M))
    _lib.check(st, "vivit_channel_scale_f32")
    return out


@_launcher
def maxpool2d_jac_t(M, x, kernel_size, stride, padding):
    """Transposed input-Jacobian of ``MaxPool2d`` (no dilation, no ceil_mode): ``M [V, N, C, OH, OW]``, ``x [N, C, H, W]``."""
    _require_device(M, x)
    M, x = M.contiguous(), x.contiguous()
    Vd, N, C, OH, OW = M.shape
    if tuple(x.shape[:2]) != (N, C):
        raise ValueError(f"x must be [{N}, {C}, H, W], got {tuple(x.shape)}")
    H, W = x.shape[2:]
    out = torch.empty((Vd, N, C, H, W), dtype=torch.float32, device=M.device)
    idx = torch.empty(N * C * OH * OW, dtype=torch.int32, device=M.device)
    st = _lib.load().vivit_maxpool2d_jac_t_f32(M.data_ptr(), x.data_ptr(), out.data_ptr(), idx.data_ptr(), Vd, N * C, H, W, OH, OW,
                                              kernel_size[0], kernel_size[1], stride[0], stride[1], padding[0], padding[1], _stream(M))
    _lib.check(st, "vivit_maxpool2d_jac_t_f32")
    return out


@_launcher
def avgpool2d_jac_t(M, in_hw, kernel_size, stride, padding):
    """Transposed input-Jacobian of ``AvgPool2d`` (count_include_pad, no ceil_mode): ``M [V, N, C, OH, OW]`` -> ``[V, N, C, H, W]``."""
    _require_device(M)
    M = M.contiguous()
    Vd, N, C, OH, OW = M.shape
    H, W = in_hw
    out = torch.empty((Vd, N, C, H, W), dtype=torch.float32, device=M.device)
    st = _lib.load().vivit_avgpool2d_jac_t_f32(M.data_ptr(), out.data_ptr(), Vd * N * C, H, W, OH, OW, kernel_size[0], kernel_size[1],
                                              stride[0], stride[1], padding[0], padding[1], _stream(M))
    _lib.check(st, "vivit_avgpool2d_jac_t_f32")
    return out


@_launcher
def conv2d_jac_t(M, weight, in_hw, stride, padding, dilation):
    """Transposed input-Jacobian of ``Conv2d`` (groups = 1, zero padding): ``M [V, N, Cout, OH, OW]``, ``weight
    [Cout, Cin, KH, KW]`` -> ``[V, N, Cin, H, W]``."""
    _require_device(M, weight)
    M, weight = M.contiguous(), weight.contiguous()
    Vd, N, Cout, OH, OW = M.shape
    Co, Cin, KH, KW = weight.shape
    if Co != Cout:
        raise ValueError(f"weight must have {Cout} output channels, got {Co}")
    H, W = in_hw
    out = torch.empty((Vd, N, Cin, H, W), dtype=torch.float32, device=M.device)
    st = _lib.load().vivit_conv2d_jac_t_f32(M.data_ptr(), weight.data_ptr(), out.data_ptr(), Vd * N, Cin, H, W, Cout, KH, KW, OH, OW,
                                           stride[0], stride[1], padding[0], padding[1], dilation[0], dilation[1], _stream(M))
    _lib.check(st, "vivit_conv2d_jac_t_f32")
    return out


@_launcher
def bn_eval_rules(M, x, scale, mean=None, rstd=None):
    """All rules of a BatchNorm in eval mode in one pass over the factor (``vivit_bn_eval_rules_f32``): ``M [V, N, C, *spatial]``,
    ``x [N, C, *spatial]`` (the module's input), ``scale [C]`` -> ``(M * scale_c  [like M], sum_l M x  [V, N, C], sum_l M  [V, N, C])``;
    with ``mean`` / ``rstd`` ``[C]`` the second result is the finished weight rule ``(sum_l M x - mean_c sum_l M) rstd_c``."""
    _require_device(M, x, scale)
    M, x, scale = M.contiguous(), x.contiguous(), scale.contiguous()
    if (mean is None) != (rstd is None):
        raise ValueError("mean and rstd come together")
    if mean is not None:
        mean, rstd = mean.contiguous(), rstd.contiguous()
    if M.dim() < 3 or tuple(M.shape[1:]) != tuple(x.shape) or scale.numel() != M.shape[2]:
        raise ValueError(f"M must be [V, *x.shape] with {scale.numel()} channels, got {tuple(M.shape)} for x {tuple(x.shape)}")
    Vd, N, C = M.shape[:3]
    L = M[0, 0, 0].numel()
    out = torch.empty_like(M)
    mx = torch.empty((Vd, N, C), dtype=torch.float32, device=M.device)
    ms = torch.empty((Vd, N, C), dtype=torch.float32, device=M.device)
    st = _lib.load().vivit_bn_eval_rules_f32(M.data_ptr(), x.data_ptr(), scale.data_ptr(), out.data_ptr(), mx.data_ptr(), ms.data_ptr(),
                                            Vd * N * C, N * C, C, L, mean.data_ptr() if mean is not None else None,
                                            rstd.data_ptr() if rstd is not None else None, _stream(M))
    _lib.check(st, "vivit_bn_eval_rules_f32")
    return out, mx, ms


@_launcher
def norm_stats(x, rows: int, eps: float):
    """``(mean [rows], rstd [rows])`` of the normalisation rows of ``x`` (``rows * L`` elements, ``vivit_norm_stats_f32``): the
    biased variance, two passes, ``rstd = 1 / sqrt(var + eps)`` -- the statistics of ``nn.LayerNorm`` / ``nn.GroupNorm``."""
    _require_device(x)
    x = x.contiguous()
    if rows <= 0 or x.numel() == 0 or x.numel() % rows != 0:
        raise ValueError(f"x must hold {rows} rows of equal length, got {tuple(x.shape)}")
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    st = _lib.load().vivit_norm_stats_f32(x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, x.numel() // rows, float(eps), _stream(x))
    _lib.check(st, "vivit_norm_stats_f32")
    return mean, rstd


@_launcher
def norm_rules(M, x, gamma, mean, rstd, groups: int = 1, seg: int = 1, want=(True, True, True)):
    """The rules of a LayerNorm / GroupNorm in one visit of every normalisation row (``vivit_norm_rules_f32``): ``M [V, *x.shape]``,
    ``x`` of ``rows = mean.numel()`` rows of ``L`` elements, ``gamma`` (``groups * L / seg`` values; ``None``: 1) ->
    ``(out [like M], seg_w [V, rows, L / seg], seg_b [V, rows, L / seg])``: the transposed input Jacobian
    ``rstd (h - mean(h) - xhat mean(h xhat))`` with ``h = gamma M``, and the sums of ``M xhat`` and of ``M`` over the ``L / seg``
    segments of ``seg`` elements of a row.  ``want``: which of the three to compute (``None`` for the others)."""
    _require_device(M, x, gamma, mean, rstd)
    M, x, mean, rstd = M.contiguous(), x.contiguous(), mean.contiguous(), rstd.contiguous()
    if M.dim() < 2 or tuple(M.shape[1:]) != tuple(x.shape):
        raise ValueError(f"M must be [V, *x.shape], got {tuple(M.shape)} for x {tuple(x.shape)}")
    rows = mean.numel()
    if rows == 0 or rstd.numel() != rows or x.numel() == 0 or x.numel() % rows != 0:
        raise ValueError(f"mean and rstd must hold one value per normalisation row of x, got {mean.numel()} and {rstd.numel()}")
    L = x.numel() // rows
    if groups <= 0 or seg <= 0 or L % seg != 0 or rows % groups != 0:
        raise ValueError(f"rows of {L} elements do not split into segments of {seg}, or {rows} rows not into {groups} groups")
    nseg = L // seg
    if gamma is not None:
        gamma = gamma.contiguous()
        if gamma.numel() != groups * nseg:
            raise ValueError(f"gamma must have {groups * nseg} elements, got {gamma.numel()}")
    if not any(want):
        raise ValueError("nothing to compute")
    Vd = M.shape[0]
    out = torch.empty_like(M) if want[0] else None
    sw = torch.empty((Vd, rows, nseg), dtype=torch.float32, device=M.device) if want[1] else None
    sb = torch.empty((Vd, rows, nseg), dtype=torch.float32, device=M.device) if want[2] else None
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    st = _lib.load().vivit_norm_rules_f32(M.data_ptr(), x.data_ptr(), ptr(gamma), mean.data_ptr(), rstd.data_ptr(), ptr(out), ptr(sw),
                                         ptr(sb), Vd, rows, L, groups, seg, _stream(M))
    _lib.check(st, "vivit_norm_rules_f32")
    return out, sw, sb


@_launcher
def norm_position_sums(M, x, mean, rstd):
    """Parameter rules of a LayerNorm with extra dimensions (``vivit_norm_position_sums_f32``): ``M [V, N, A, D]``, ``x [N, A, D]``,
    ``mean`` / ``rstd`` of ``N * A`` values -> ``(sum_a M xhat, sum_a M)``, both ``[V, N, D]``."""
    _require_device(M, x, mean, rstd)
    M, x, mean, rstd = M.contiguous(), x.contiguous(), mean.contiguous(), rstd.contiguous()
    if M.dim() != 4 or tuple(M.shape[1:]) != tuple(x.shape):
        raise ValueError(f"M must be [V, N, A, D] and x [N, A, D], got {tuple(M.shape)} for x {tuple(x.shape)}")
    Vd, N, A, D = M.shape
    if mean.numel() != N * A or rstd.numel() != N * A:
        raise ValueError(f"mean and rstd must have {N * A} elements, got {mean.numel()} and {rstd.numel()}")
    pw = torch.empty((Vd, N, D), dtype=torch.float32, device=M.device)
    pb = torch.empty((Vd, N, D), dtype=torch.float32, device=M.device)
    st = _lib.load().vivit_norm_position_sums_f32(M.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), pw.data_ptr(), pb.data_ptr(),
                                                 Vd, N, A, D, _stream(M))
    _lib.check(st, "vivit_norm_position_sums_f32")
    return pw, pb


def _out_like(out, ref, what: str):
    """``out`` (a caller's buffer for a result shaped like ``ref``) checked, or a new tensor."""
    if out is None:
        return torch.empty(tuple(ref.shape), dtype=torch.float32, device=ref.device)
    _require_device(out)
    if tuple(out.shape) != tuple(ref.shape) or not out.is_contiguous() or out.device != ref.device:
        raise ValueError(f"{what} must be a contiguous tensor of shape {tuple(ref.shape)} on {ref.device}")
    return out


@_launcher
def rms_norm_stats(x, rows: int, eps: float):
    """``rstd [rows]`` of the normalisation rows of ``x`` (``rows * L`` elements, ``vivit_rms_norm_stats_f32``):
    ``1 / sqrt(mean(x^2) + eps)`` -- the statistic of ``nn.RMSNorm``."""
    _require_device(x)
    x = x.contiguous()
    if rows <= 0 or x.numel() == 0 or x.numel() % rows != 0:
        raise ValueError(f"x must hold {rows} rows of equal length, got {tuple(x.shape)}")
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    st = _lib.load().vivit_rms_norm_stats_f32(x.data_ptr(), rstd.data_ptr(), rows, x.numel() // rows, float(eps), _stream(x))
    _lib.check(st, "vivit_rms_norm_stats_f32")
    return rstd


@_launcher
def rms_norm_rules(M, x, gamma, rstd, want=(True, True), out=None, w=None):
    """The rules of an RMSNorm in one visit of every normalisation row (``vivit_rms_norm_rules_f32``): ``M [V, *x.shape]``, ``x`` of
    ``rows = rstd.numel()`` rows of ``L`` elements, ``gamma`` (``L`` values; ``None``: 1) -> ``(out, w)``, both like ``M``: the
    transposed input Jacobian ``rstd (h - xhat mean(h xhat))`` with ``h = gamma M``, ``xhat = x rstd``, and ``M xhat``.  ``want``:
    which of the two to compute (``None`` for the other); ``out`` / ``w``: buffers to write them to."""
    _require_device(M, x, gamma, rstd)
    M, x, rstd = M.contiguous(), x.contiguous(), rstd.contiguous()
    if M.dim() < 2 or tuple(M.shape[1:]) != tuple(x.shape):
        raise ValueError(f"M must be [V, *x.shape], got {tuple(M.shape)} for x {tuple(x.shape)}")
    rows = rstd.numel()
    if rows == 0 or x.numel() == 0 or x.numel() % rows != 0:
        raise ValueError(f"rstd must hold one value per normalisation row of x, got {rows} for x {tuple(x.shape)}")
    L = x.numel() // rows
    if gamma is not None:
        gamma = gamma.contiguous()
        if gamma.numel() != L:
            raise ValueError(f"gamma must have {L} elements, got {gamma.numel()}")
    if not any(want):
        raise ValueError("nothing to compute")
    out = _out_like(out, M, "out") if want[0] else None
    w = _out_like(w, M, "w") if want[1] else None
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    st = _lib.load().vivit_rms_norm_rules_f32(M.data_ptr(), x.data_ptr(), ptr(gamma), rstd.data_ptr(), ptr(out), ptr(w), M.shape[0], rows, L,
                                             _stream(M))
    _lib.check(st, "vivit_rms_norm_rules_f32")
    return out, w


@_launcher
def rms_norm_position_sums(M, x, rstd, out=None):
    """Weight rule of an RMSNorm with extra dimensions (``vivit_rms_norm_position_sums_f32``): ``M [V, N, A, D]``, ``x [N, A, D]``,
    ``rstd`` of ``N * A`` values -> ``sum_a M x rstd  [V, N, D]``."""
    _require_device(M, x, rstd)
    M, x, rstd = M.contiguous(), x.contiguous(), rstd.contiguous()
    if M.dim() != 4 or tuple(M.shape[1:]) != tuple(x.shape) or M.numel() == 0:
        raise ValueError(f"M must be [V, N, A, D] and x [N, A, D], got {tuple(M.shape)} for x {tuple(x.shape)}")
    Vd, N, A, D = M.shape
    if rstd.numel() != N * A:
        raise ValueError(f"rstd must have {N * A} elements, got {rstd.numel()}")
    pw = _out_like(out, M[:, :, 0], "out")
    st = _lib.load().vivit_rms_norm_position_sums_f32(M.data_ptr(), x.data_ptr(), rstd.data_ptr(), pw.data_ptr(), Vd, N, A, D, _stream(M))
    _lib.check(st, "vivit_rms_norm_position_sums_f32")
    return pw


@_launcher
def gate_jac_t(M, a, b, want=(True, True), out_a=None, out_b=None):
    """Transposed input Jacobians of the product ``a * b`` (``vivit_gate_jac_t_f32``): ``M [V, *a.shape]`` -> ``(M b, M a)``, the
    factors handed to ``a`` and to ``b``, from one read of ``M``.  ``want``: which of the two to compute (``None`` for the other,
    whose operand may be ``None`` as well); ``out_a`` / ``out_b``: buffers to write them to."""
    _require_device(M, a, b)
    M = M.contiguous()
    if not any(want):
        raise ValueError("nothing to compute")
    for t, needed, name in ((b, want[0], "b"), (a, want[1], "a")):
        if needed and (t is None or M.dim() < 1 or tuple(M.shape[1:]) != tuple(t.shape)):
            raise ValueError(f"M must be [V, *{name}.shape], got {tuple(M.shape)} for {name} {None if t is None else tuple(t.shape)}")
    if M.numel() == 0:
        raise ValueError(f"empty operands: M {tuple(M.shape)}")
    a = a.contiguous() if want[1] else None
    b = b.contiguous() if want[0] else None
    Ga = _out_like(out_a, M, "out_a") if want[0] else None
    Gb = _out_like(out_b, M, "out_b") if want[1] else None
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    st = _lib.load().vivit_gate_jac_t_f32(M.data_ptr(), ptr(a), ptr(b), ptr(Ga), ptr(Gb), M.shape[0], M.numel() // M.shape[0], _stream(M))
    _lib.check(st, "vivit_gate_jac_t_f32")
    return Ga, Gb


def _packed_heads(num_heads, num_kv_heads):
    """``(Hkv, text)`` of a packed projection ``[..., (num_heads + 2 Hkv) * d]``: the key / value heads, checked -- ``num_heads`` query
    heads in ``num_kv_heads`` groups of consecutive heads; ``None`` is multi-head attention, ``Hkv = num_heads`` -- and how the
    messages write the number of heads."""
    if num_kv_heads is None:
        return num_heads, f"3 * {num_heads}"
    if num_heads < 1 or num_kv_heads < 1 or num_heads % num_kv_heads != 0:
        raise ValueError(f"num_heads H = {num_heads} must be a positive multiple of num_kv_heads Hkv = {num_kv_heads} >= 1")
    return num_kv_heads, f"({num_heads} + 2 * {num_kv_heads})"


@_launcher
def rope_jac_t(M, cos, sin, num_heads: int, out=None, num_kv_heads: int = None):
    """Transposed Jacobian of the rotary position embedding on a packed projection (``vivit_rope_gqa_jac_t_f32``): ``M [..., T, 3 E]``
    (``E = num_heads * d``), ``cos`` / ``sin [T, d / 2]`` -> like ``M``: the q and k thirds rotated back, the v third copied.
    ``out``: a buffer for the result; ``M`` itself for the rule in place.  ``num_kv_heads`` (grouped-query attention; ``None`` is
    ``num_heads``, the three thirds): ``M [..., T, (num_heads + 2 * num_kv_heads) * d]``, the ``num_heads + num_kv_heads`` heads of
    the q and k parts rotated back, the v part copied."""
    _require_device(M, cos, sin)
    if out is M and not M.is_contiguous():
        raise ValueError("the rule in place needs a contiguous M")
    M, cos, sin = M.contiguous(), cos.contiguous(), sin.contiguous()
    Hkv, heads_text = _packed_heads(num_heads, num_kv_heads)
    heads = num_heads + 2 * Hkv
    if M.dim() < 2 or num_heads < 1 or M.shape[-1] == 0 or M.shape[-1] % (2 * heads) != 0:
        raise ValueError(f"M must be [..., T, {heads_text} heads * an even head dimension], got {tuple(M.shape)}")
    T, d = M.shape[-2], M.shape[-1] // heads
    if tuple(cos.shape) != (T, d // 2) or tuple(sin.shape) != (T, d // 2):
        raise ValueError(f"cos and sin must be {(T, d // 2)}, got {tuple(cos.shape)} and {tuple(sin.shape)}")
    if M.numel() == 0:
        raise ValueError(f"empty operands: M {tuple(M.shape)}")
    G = _out_like(out, M, "out")
    if G is not M and G.untyped_storage().data_ptr() == M.untyped_storage().data_ptr():
        lo, hi = G.data_ptr(), G.data_ptr() + 4 * G.numel()
        if M.data_ptr() < hi and lo < M.data_ptr() + 4 * M.numel() and G.data_ptr() != M.data_ptr():
            raise ValueError("out must be M itself or must not overlap it")
    rows = M.numel() // (T * M.shape[-1])
    st = _lib.load().vivit_rope_gqa_jac_t_f32(M.data_ptr(), cos.data_ptr(), sin.data_ptr(), G.data_ptr(), rows, T, num_heads, Hkv, d, _stream(M))
    _lib.check(st, "vivit_rope_gqa_jac_t_f32")
    return G


def _softcap(cap) -> float:
    """A logit cap, checked: a finite float ``> 0``."""
    if isinstance(cap, bool) or not isinstance(cap, (int, float)) or not (cap > 0) or math.isinf(cap):
        raise ValueError(f"softcap must be a finite float > 0, got {cap!r}")
    return float(cap)


@_launcher
def attention_jac_t(M, qkv, out, num_heads: int, scale: float, causal: bool, num_kv_heads: int = None, lengths=None, window: int = None,
                    softcap: float = None, bias=None):
    """Transposed input Jacobian of scaled dot-product self-attention (``vivit_attention_masked_jac_t_f32``, the one entry that
    launches): ``M [V, N, T, E]`` (the factor at the module output), ``qkv [N, T, 3 E]`` (the module input, q | k | v), ``out [N, T, E]``
    (the module output of the forward pass) -> ``[V, N, T, 3 E]``.  ``E = num_heads * d``; no ``T x T`` tensor is allocated.
    ``num_kv_heads`` (grouped-query attention; ``None`` is ``num_heads``, the three thirds): ``qkv [N, T, (num_heads + 2 *
    num_kv_heads) * d]``, query head ``h`` attends to key / value head ``h // (num_heads // num_kv_heads)``; the result is packed
    ``dQ | dK | dV`` like ``qkv``.

    ``lengths`` (anything ``torch.as_tensor`` turns into ``N`` integers): sample ``n`` has the positions ``0 .. lengths[n] - 1``
    (right padding; the kernel clamps to ``[0, T]``).  The positions beyond are dead: invisible as keys, rows of exact zeros in the
    result, and whatever ``M``, ``qkv`` and ``out`` hold there is never read.  The values go to ``M``'s device as int32 and are not
    looked at on the host.  ``window`` (an integer ``>= 1``): query ``i`` sees the keys with ``|i - j| < window`` (with ``causal`` the
    ``window`` keys up to and including its own).  With both ``None`` (a null pointer and ``window = 0`` for the entry) the kernels
    walk every key block unmasked: what the entries without them, ``vivit_attention_jac_t_f32`` and
    ``vivit_attention_gqa_jac_t_f32``, hand to the same entry.

    ``softcap`` (a finite float ``c > 0``) and ``bias`` (a float32 tensor ``[num_heads, 2 T - 1]`` on ``M``'s device): the score
    function ``s_ij = c tanh(scale q_i k_j / c) + bias[h, j - i + T - 1]`` (either part alone where only one is given), the cap before
    the bias and both before the mask; the table is a constant of this rule (a learned table's own factor:
    :func:`attention_bias_factor`).  With either the call goes to
    ``vivit_attention_scoremod_jac_t_f32``; with both ``None`` it is the call above, unchanged."""
    if softcap is not None:
        softcap = _softcap(softcap)
    _require_device(M, qkv, out)
    if bias is not None:
        _require_device(bias)
        if bias.dtype != torch.float32 or bias.device != M.device:
            raise ValueError(f"bias must be a float32 tensor on {M.device}, got {bias.dtype} on {bias.device}")
        bias = bias.contiguous()
    if window is not None and (isinstance(window, bool) or int(window) != window or window < 1):
        raise ValueError(f"window must be an integer >= 1 (or None), got {window!r}")
    if lengths is not None:
        lengths = torch.as_tensor(lengths)
        if lengths.is_floating_point() or lengths.is_complex() or lengths.dtype == torch.bool:
            raise ValueError(f"lengths must be integers, got {lengths.dtype}")
        if lengths.dim() != 1 or qkv.dim() != 3 or lengths.shape[0] != qkv.shape[0]:
            raise ValueError(f"lengths must be [N] = [{qkv.shape[0] if qkv.dim() == 3 else '?'}], got {tuple(lengths.shape)}")
        lengths = lengths.to(device=M.device, dtype=torch.int32).contiguous()
    M, qkv, out = M.contiguous(), qkv.contiguous(), out.contiguous()
    Hkv, heads_text = _packed_heads(num_heads, num_kv_heads)
    heads = num_heads + 2 * Hkv
    if qkv.dim() != 3 or num_heads < 1 or qkv.shape[2] == 0 or qkv.shape[2] % heads != 0:
        raise ValueError(f"qkv must be [N, T, {heads_text} * d], got {tuple(qkv.shape)}")
    N, T, E3 = qkv.shape
    d = E3 // heads
    E = num_heads * d
    if tuple(out.shape) != (N, T, E):
        raise ValueError(f"out must be {(N, T, E)}, got {tuple(out.shape)}")
    if M.dim() != 4 or tuple(M.shape[1:]) != (N, T, E):
        raise ValueError(f"M must be [V, {N}, {T}, {E}], got {tuple(M.shape)}")
    Vd = M.shape[0]
    if Vd == 0 or N == 0 or T == 0:
        raise ValueError(f"empty operands: M {tuple(M.shape)}")
    if bias is not None and tuple(bias.shape) != (num_heads, 2 * T - 1):
        raise ValueError(f"bias must be [H, 2 T - 1] = {(num_heads, 2 * T - 1)}, got {tuple(bias.shape)}")
    G = torch.empty((Vd, N, T, E3), dtype=torch.float32, device=M.device)
    lib = _lib.load()
    if softcap is not None or bias is not None:
        ws, ws_bytes = _workspace(lib.vivit_attention_scoremod_jac_t_f32_workspace_bytes(Vd, N, T, num_heads, Hkv, d), M)
        st = lib.vivit_attention_scoremod_jac_t_f32(M.data_ptr(), qkv.data_ptr(), out.data_ptr(), G.data_ptr(), Vd, N, T, num_heads, Hkv, d,
                                                    float(scale), int(bool(causal)), None if lengths is None else lengths.data_ptr(),
                                                    0 if window is None else int(window), 0.0 if softcap is None else softcap,
                                                    None if bias is None else bias.data_ptr(), ws, ws_bytes, _stream(M))
        _lib.check(st, "vivit_attention_scoremod_jac_t_f32")
        return G
    ws, ws_bytes = _workspace(lib.vivit_attention_masked_jac_t_f32_workspace_bytes(Vd, N, T, num_heads, Hkv, d), M)
    st = lib.vivit_attention_masked_jac_t_f32(M.data_ptr(), qkv.data_ptr(), out.data_ptr(), G.data_ptr(), Vd, N, T, num_heads, Hkv, d,
                                              float(scale), int(bool(causal)), None if lengths is None else lengths.data_ptr(),
                                              0 if window is None else int(window), ws, ws_bytes, _stream(M))
    _lib.check(st, "vivit_attention_masked_jac_t_f32")
    return G


@_launcher
def attention_bias_factor(M, qkv, out, num_heads: int, scale: float, causal: bool, bias, index=None, width: int = None,
                          num_kv_heads: int = None, lengths=None, window: int = None, softcap: float = None):
    """The factor of a learned relative-position table of scaled dot-product self-attention (``vivit_attention_bias_factor_f32``):
    ``M [V, N, T, E]``, ``qkv``, ``out``, ``num_kv_heads``, ``lengths``, ``window`` and ``softcap`` as :func:`attention_jac_t` has
    them, ``bias`` the EFFECTIVE table ``[num_heads, 2 T - 1]`` of the ``T`` positions (float32 on ``M``'s device) ->
    ``[V, N, num_heads, width]``: column ``b`` is the sum of ``dS[v, n, h, i, j]`` over the visible pairs whose distance ``r = j - i``
    has ``index[r + T - 1] == b``.  ``index`` (``2 T - 1`` integers, anything ``torch.as_tensor`` takes; it goes to ``M``'s device as
    int32 and is not looked at on the host) sends distances to columns, ``width`` is the number of columns: a table built for
    ``L >= T`` positions passes ``index[k] = k + (L - T)`` and ``width = 2 L - 1``, a table indexed through buckets the middle slice
    of its bucket map and the number of buckets.  A value outside ``[0, width)`` is skipped by the kernel.  ``index=None`` is the
    identity map of a ``[H, 2 T - 1]`` table (``width`` must then be ``None`` or ``2 T - 1``).  No ``T x T`` tensor is allocated, no
    atomics: the bytes of the result are a function of the operands."""
    if softcap is not None:
        softcap = _softcap(softcap)
    _require_device(M, qkv, out, bias)
    if bias.dtype != torch.float32 or bias.device != M.device:
        raise ValueError(f"bias must be a float32 tensor on {M.device}, got {bias.dtype} on {bias.device}")
    if window is not None and (isinstance(window, bool) or int(window) != window or window < 1):
        raise ValueError(f"window must be an integer >= 1 (or None), got {window!r}")
    if lengths is not None:
        lengths = _device_lengths(lengths, "lengths", qkv.shape[0] if qkv.dim() == 3 else None, M.device)
    M, qkv, out, bias = M.contiguous(), qkv.contiguous(), out.contiguous(), bias.contiguous()
    Hkv, heads_text = _packed_heads(num_heads, num_kv_heads)
    heads = num_heads + 2 * Hkv
    if qkv.dim() != 3 or num_heads < 1 or qkv.shape[2] == 0 or qkv.shape[2] % heads != 0:
        raise ValueError(f"qkv must be [N, T, {heads_text} * d], got {tuple(qkv.shape)}")
    N, T, E3 = qkv.shape
    d = E3 // heads
    E = num_heads * d
    if tuple(out.shape) != (N, T, E):
        raise ValueError(f"out must be {(N, T, E)}, got {tuple(out.shape)}")
    if M.dim() != 4 or tuple(M.shape[1:]) != (N, T, E):
        raise ValueError(f"M must be [V, {N}, {T}, {E}], got {tuple(M.shape)}")
    Vd = M.shape[0]
    if Vd == 0 or N == 0 or T == 0:
        raise ValueError(f"empty operands: M {tuple(M.shape)}")
    if tuple(bias.shape) != (num_heads, 2 * T - 1):
        raise ValueError(f"bias must be [H, 2 T - 1] = {(num_heads, 2 * T - 1)}, got {tuple(bias.shape)}")
    if index is None:
        if width is not None and width != 2 * T - 1:
            raise ValueError(f"width must be 2 T - 1 = {2 * T - 1} (or None) without an index, got {width!r}")
        index, width = torch.arange(2 * T - 1, dtype=torch.int32, device=M.device), 2 * T - 1
    else:
        index = torch.as_tensor(index)
        if index.is_floating_point() or index.is_complex() or index.dtype == torch.bool:
            raise ValueError(f"index must be integers, got {index.dtype}")
        if tuple(index.shape) != (2 * T - 1,):
            raise ValueError(f"index must be [2 T - 1] = [{2 * T - 1}], got {tuple(index.shape)}")
        if width is None or isinstance(width, bool) or int(width) != width or width < 1:
            raise ValueError(f"width must be an integer >= 1 with an index, got {width!r}")
        index, width = index.to(device=M.device, dtype=torch.int32).contiguous(), int(width)
    Gb = torch.empty((Vd, N, num_heads, width), dtype=torch.float32, device=M.device)
    lib = _lib.load()
    ws, ws_bytes = _workspace(lib.vivit_attention_bias_factor_f32_workspace_bytes(Vd, N, T, num_heads, Hkv, d), M)
    st = lib.vivit_attention_bias_factor_f32(M.data_ptr(), qkv.data_ptr(), out.data_ptr(), Gb.data_ptr(), Vd, N, T, num_heads, Hkv, d,
                                             float(scale), int(bool(causal)), None if lengths is None else lengths.data_ptr(),
                                             0 if window is None else int(window), 0.0 if softcap is None else softcap,
                                             bias.data_ptr(), index.data_ptr(), width, ws, ws_bytes, _stream(M))
    _lib.check(st, "vivit_attention_bias_factor_f32")
    return Gb


def _device_lengths(lengths, name: str, N, device):
    """``lengths`` (anything ``torch.as_tensor`` turns into ``N`` integers) as int32 on ``device``, never read on the host."""
    lengths = torch.as_tensor(lengths)
    if lengths.is_floating_point() or lengths.is_complex() or lengths.dtype == torch.bool:
        raise ValueError(f"{name} must be integers, got {lengths.dtype}")
    if lengths.dim() != 1 or N is None or lengths.shape[0] != N:
        raise ValueError(f"{name} must be [N] = [{'?' if N is None else N}], got {tuple(lengths.shape)}")
    return lengths.to(device=device, dtype=torch.int32).contiguous()


@_launcher
def cross_attention_jac_t(M, q, kv, out, num_heads: int, scale: float, num_kv_heads: int = None, query_lengths=None, key_lengths=None,
                          want=(True, True)):
    """Transposed input Jacobians of scaled dot-product cross-attention (``vivit_attention_cross_jac_t_f32``): ``M [V, N, Tq, E]`` (the
    factor at the module output), ``q [N, Tq, E]`` (the queries, ``E = num_heads * d``), ``kv [N, Tk, 2 * Hkv * d]`` (the second
    sequence, k | v: ``Hkv`` key heads, then ``Hkv`` value heads; ``Hkv = num_kv_heads``, ``None`` is ``num_heads``), ``out [N, Tq, E]``
    (the module output of the forward pass) -> ``(Gq [V, N, Tq, E], Gkv [V, N, Tk, 2 * Hkv * d])``, ``Gkv`` packed ``dK | dV`` like
    ``kv``.  Query head ``h`` attends to key / value head ``h // (num_heads // Hkv)``; no ``Tq x Tk`` tensor is allocated.

    There is no causal mask and no window: with ``Tq != Tk`` there is no agreed alignment of the diagonal.  ``query_lengths`` /
    ``key_lengths`` (each anything ``torch.as_tensor`` turns into ``N`` integers, or ``None``): right padding, clamped by the kernel
    to ``[0, Tq]`` and ``[0, Tk]``.  Key ``j`` of sample ``n`` is live iff ``j < key_lengths[n]``; query ``i`` iff
    ``i < query_lengths[n]`` and ``key_lengths[n] > 0`` (a query with no key to look at is dead, not a NaN).  Dead rows of both
    results are exact zeros, and whatever ``M``, ``q``, ``kv`` and ``out`` hold at dead positions is never read.  The values go to
    ``M``'s device as int32 and are not looked at on the host.

    ``want``: which of the two results to compute; the other is ``None`` and its kernel is not launched (``want=(True, False)``: a
    frozen memory that needs no gradient)."""
    _require_device(M, q, kv, out)
    want = tuple(bool(w) for w in want)
    if len(want) != 2 or not any(want):
        raise ValueError(f"want must name at least one of (Gq, Gkv), got {want!r}")
    N0 = q.shape[0] if q.dim() == 3 else None
    if query_lengths is not None:
        query_lengths = _device_lengths(query_lengths, "query_lengths", N0, M.device)
    if key_lengths is not None:
        key_lengths = _device_lengths(key_lengths, "key_lengths", N0, M.device)
    M, q, kv, out = M.contiguous(), q.contiguous(), kv.contiguous(), out.contiguous()
    Hkv, _ = _packed_heads(num_heads, num_kv_heads)
    if q.dim() != 3 or num_heads < 1 or q.shape[2] == 0 or q.shape[2] % num_heads != 0:
        raise ValueError(f"q must be [N, Tq, {num_heads} * d], got {tuple(q.shape)}")
    N, Tq, E = q.shape
    d = E // num_heads
    if kv.dim() != 3 or kv.shape[0] != N or kv.shape[2] != 2 * Hkv * d:
        raise ValueError(f"kv must be [{N}, Tk, 2 * {Hkv} * {d}], got {tuple(kv.shape)}")
    Tk = kv.shape[1]
    if tuple(out.shape) != (N, Tq, E):
        raise ValueError(f"out must be {(N, Tq, E)}, got {tuple(out.shape)}")
    if M.dim() != 4 or tuple(M.shape[1:]) != (N, Tq, E):
        raise ValueError(f"M must be [V, {N}, {Tq}, {E}], got {tuple(M.shape)}")
    Vd = M.shape[0]
    if Vd == 0 or N == 0 or Tq == 0 or Tk == 0:
        raise ValueError(f"empty operands: M {tuple(M.shape)}, kv {tuple(kv.shape)}")
    Gq = torch.empty((Vd, N, Tq, E), dtype=torch.float32, device=M.device) if want[0] else None
    Gkv = torch.empty((Vd, N, Tk, 2 * Hkv * d), dtype=torch.float32, device=M.device) if want[1] else None
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    lib = _lib.load()
    ws, ws_bytes = _workspace(lib.vivit_attention_cross_jac_t_f32_workspace_bytes(Vd, N, Tq, Tk, num_heads, Hkv, d), M)
    st = lib.vivit_attention_cross_jac_t_f32(M.data_ptr(), q.data_ptr(), kv.data_ptr(), out.data_ptr(), ptr(Gq), ptr(Gkv), Vd, N, Tq, Tk,
                                             num_heads, Hkv, d, float(scale), ptr(query_lengths), ptr(key_lengths), ws, ws_bytes,
                                             _stream(M))
    _lib.check(st, "vivit_attention_cross_jac_t_f32")
    return Gq, Gkv


_I32_MAX = 2 ** 31 - 1


def embedding_token_slots(idx, padding_idx=None):
    """The slots of the compact form of an Embedding's weight factor, from the token ids ``idx [N, T]`` (any integer dtype) -- torch
    ops on the device of ``idx``, no host synchronisation (plumbing shared by :func:`embedding_compact` and the torch rule of
    non-HIP tensors).  Returns ``(ids, perm, seg_start, seg_count, slot_of_t)``, all ``[N, T]``: ``ids`` (int32) holds sample n's
    distinct tokens in strictly increasing order and -1 in the unused slots; ``perm`` (int32) the positions ``t`` ordered by token,
    stably; slot ``u`` owns the ``seg_count[n, u]`` sorted positions from ``seg_start[n, u]`` on (int32); ``slot_of_t`` (int64) is the
    slot of position ``t``, ``T`` for a padding position.  Padding positions are sorted under the key 2^31 - 1, which no token the
    kernels accept can have (ids are int32 and below ``num_embeddings``)."""
    N, T = idx.shape
    key = idx.to(torch.int64)
    if padding_idx is not None:
        key = key.masked_fill(key == padding_idx, _I32_MAX)       # padding sorts behind every token
    sk, perm = torch.sort(key, dim=1, stable=True)
    valid = sk != _I32_MAX if padding_idx is not None else torch.ones_like(sk, dtype=torch.bool)
    new = torch.ones_like(valid)
    new[:, 1:] = sk[:, 1:] != sk[:, :-1]
    slot = new.cumsum(1) - 1                                      # slot of every sorted position
    ids = torch.full((N, T), -1, dtype=torch.int64, device=idx.device)
    ids.scatter_(1, slot, sk.masked_fill(~valid, -1))             # (the writes that meet in a slot carry the same value)
    cnt = torch.zeros((N, T), dtype=torch.int64, device=idx.device).scatter_add_(1, slot, valid.to(torch.int64))
    start = cnt.cumsum(1) - cnt
    slot_of_t = torch.empty_like(slot).scatter_(1, perm, slot.masked_fill(~valid, T))
    return ids.to(torch.int32), perm.to(torch.int32), start.to(torch.int32), cnt.to(torch.int32), slot_of_t


def _embedding_operands(B, ids):
    _require_device(B)
    if B.dim() != 4 or B.numel() == 0:
        raise ValueError(f"B must be a non-empty [V, N, T, D] tensor, got {tuple(B.shape)}")
    if not ids.is_cuda or ids.device != B.device or ids.dtype != torch.int32 or tuple(ids.shape) != tuple(B.shape[1:3]):
        raise ValueError(f"ids must be an int32 [{B.shape[1]}, {B.shape[2]}] tensor on {B.device}, got {ids.dtype} {tuple(ids.shape)} on {ids.device}")
    return B.contiguous(), ids.contiguous()


@_launcher
def embedding_compact(M, idx, padding_idx=None):
    """Compact form of an Embedding's weight factor (``vivit_embedding_compact_f32``): ``M [V, N, T, D]`` (the factor at the module
    output), ``idx [N, T]`` (integer token ids) -> ``(B [V, N, T, D], ids [N, T] int32)``.  ``ids[n]``: sample n's distinct tokens,
    strictly increasing, then -1; ``B[v, n, u]``: the sum of the rows of ``M[v, n]`` whose token is ``ids[n, u]`` in ascending ``t``,
    zero for a -1 slot.  Positions with ``idx == padding_idx`` contribute nothing.  The per-sample sort is torch's, on the device."""
    _require_device(M)
    if M.dim() != 4 or M.numel() == 0:
        raise ValueError(f"M must be a non-empty [V, N, T, D] tensor, got {tuple(M.shape)}")
    if idx.is_floating_point() or idx.device != M.device or tuple(idx.shape) != tuple(M.shape[1:3]):
        raise ValueError(f"idx must be an integer [{M.shape[1]}, {M.shape[2]}] tensor on {M.device}, got {idx.dtype} {tuple(idx.shape)} on {idx.device}")
    M = M.contiguous()
    V, N, T, D = M.shape
    ids, perm, start, cnt, _ = embedding_token_slots(idx, padding_idx)
    B = torch.empty_like(M)
    st = _lib.load().vivit_embedding_compact_f32(M.data_ptr(), perm.data_ptr(), start.data_ptr(), cnt.data_ptr(), B.data_ptr(), V, N, T, D,
                                                 _stream(M))
    _lib.check(st, "vivit_embedding_compact_f32")
    return B, ids


@_launcher
def embedding_gram(B, ids, out=None, alpha: float = 1.0, beta: float = 0.0):
    """``out = alpha * G + beta * out`` with the Gram matrix ``G [V N, V N]`` (rows ``v N + n``) of an Embedding's weight factor from
    its compact form (``vivit_embedding_gram_f32``): ``G[(v, n), (v', n')] = sum_{u, u'} [ids[n, u] = ids[n', u'] >= 0]
    <B[v, n, u], B[v', n', u']>``.  Exactly symmetric; exact zeros for samples without a common token; no tensor with an axis of
    length ``num_embeddings``."""
    B, ids = _embedding_operands(B, ids)
    _require_device(out)
    V, N, T, D = B.shape
    n = V * N
    if out is None:
        out = torch.empty((n, n), dtype=torch.float32, device=B.device)
        beta = 0.0
    if not out.is_contiguous() or tuple(out.shape) != (n, n):
        raise ValueError(f"out must be a contiguous [{n}, {n}] matrix")
    _check_out(out, n, n, B)
    lib = _lib.load()
    ws, ws_bytes = _workspace(lib.vivit_embedding_gram_f32_workspace_bytes(V, N, T, D), B)
    st = lib.vivit_embedding_gram_f32(B.data_ptr(), ids.data_ptr(), out.data_ptr(), V, N, T, D, alpha, beta, ws, ws_bytes, _stream(B))
    _lib.check(st, "vivit_embedding_gram_f32")
    return out


@_launcher
def embedding_vmp(B, ids, mat, W: int):
    """``out[f, w, :] = sum_{v, n, u: ids[n, u] = w} mat[f, v, n] * B[v, n, u, :]`` (``vivit_embedding_vmp_f32``): ``mat [F, V, N]`` ->
    ``[F, W, D]``, rows of absent tokens zero.  The token-major member list (a stable sort of the entries by token) is torch's."""
    B, ids = _embedding_operands(B, ids)
    _require_device(mat)
    V, N, T, D = B.shape
    if mat.dim() != 3 or tuple(mat.shape[1:]) != (V, N) or mat.shape[0] == 0 or W < 1:
        raise ValueError(f"mat must be [F, {V}, {N}] with F >= 1 and W >= 1, got {tuple(mat.shape)}, W = {W}")
    mat = mat.contiguous()
    F_ = mat.shape[0]
    flat = ids.reshape(-1).to(torch.int64)
    sk, order = torch.sort(flat.masked_fill(flat < 0, W), stable=True)
    tok_start = torch.searchsorted(sk, torch.arange(W + 1, device=B.device)).to(torch.int32)
    order = order.to(torch.int32)
    out = torch.empty((F_, W, D), dtype=torch.float32, device=B.device)
    st = _lib.load().vivit_embedding_vmp_f32(B.data_ptr(), order.data_ptr(), tok_start.data_ptr(), mat.data_ptr(), out.data_ptr(), F_, V, N, T,
                                             D, W, _stream(B))
    _lib.check(st, "vivit_embedding_vmp_f32")
    return out


@_launcher
def embedding_vtmp(B, ids, mat):
    """``out[f, v, n] = sum_u <mat[f, ids[n, u], :], B[v, n, u, :]>`` (``vivit_embedding_vtmp_f32``): ``mat [F, W, D]`` -> ``[F, V, N]``."""
    B, ids = _embedding_operands(B, ids)
    _require_device(mat)
    V, N, T, D = B.shape
    if mat.dim() != 3 or mat.shape[2] != D or mat.shape[0] == 0 or mat.shape[1] == 0:
        raise ValueError(f"mat must be a non-empty [F, W, {D}] tensor, got {tuple(mat.shape)}")
    mat = mat.contiguous()
    F_, W = mat.shape[:2]
    out = torch.empty((F_, V, N), dtype=torch.float32, device=B.device)
    st = _lib.load().vivit_embedding_vtmp_f32(B.data_ptr(), ids.data_ptr(), mat.data_ptr(), out.data_ptr(), F_, V, N, T, D, W, _stream(B))
    _lib.check(st, "vivit_embedding_vtmp_f32")
    return out


@_launcher
def embedding_weight_mjp(B, ids, W: int):
    """The explicit weight factor ``[V, N, W, D]`` of an Embedding from its compact form (``vivit_embedding_weight_mjp_f32``): zeros,
    then ``out[v, n, ids[n, u]] = B[v, n, u]``."""
    B, ids = _embedding_operands(B, ids)
    V, N, T, D = B.shape
    if W < 1:
        raise ValueError(f"W must be positive, got {W}")
    out = torch.empty((V, N, W, D), dtype=torch.float32, device=B.device)
    st = _lib.load().vivit_embedding_weight_mjp_f32(B.data_ptr(), ids.data_ptr(), out.data_ptr(), V, N, T, D, W, _stream(B))
    _lib.check(st, "vivit_embedding_weight_mjp_f32")
    return out


@_launcher
def row_dot(M, X=None, rows_x: int = 1):
    """``out[r] = sum_l M[r, l] * (X[r % rows_x, l] if X is given else 1)`` for ``M [rows, L]`` (fixed summation order)."""
    _require_device(M, X)
    M = _as2d(M.contiguous())
    if X is not None:
        X = _as2d(X.contiguous())
        if X.shape != (rows_x, M.shape[1]):
            raise ValueError(f"X must be [{rows_x}, {M.shape[1]}], got {tuple(X.shape)}")
    out = torch.empty(M.shape[0], dtype=torch.float32, device=M.device)
    st = _lib.load().vivit_row_dot_f32(M.data_ptr(), X.data_ptr() if X is not None else None, out.data_ptr(), M.shape[0], rows_x,
                                      M.shape[1], _stream(M))
    _lib.check(st, "vivit_row_dot_f32")
    return out


@_launcher
def ce_sqrt_hessian(logits, scale: float, onehot=None):
    """Cross-entropy loss-Hessian square root ``S [V, N, C]`` from ``logits [N, C]``: exact (``V = C``) or, with
    ``onehot [M, N, C]``, the sampled factor ``(p - onehot) * scale``."""
    _require_device(logits, onehot)
    logits = logits.contiguous()
    N, C = logits.shape
    Vd = C if onehot is None else onehot.shape[0]
    if onehot is not None:
        onehot = onehot.contiguous()
        if tuple(onehot.shape[1:]) != (N, C):
            raise ValueError(f"onehot must be [M, {N}, {C}], got {tuple(onehot.shape)}")
    S = torch.empty((Vd, N, C), dtype=torch.float32, device=logits.device)
    st = _lib.load().vivit_ce_sqrt_hessian_f32(logits.data_ptr(), onehot.data_ptr() if onehot is not None else None, S.data_ptr(), N, C,
                                              Vd, float(scale), _stream(logits))
    _lib.check(st, "vivit_ce_sqrt_hessian_f32")
    return S


@_launcher
def ce_sqrt_hessian_positions(logits, scale: float, idx=None):
    """Cross-entropy loss-Hessian square root for ``logits [N, C, *D]`` (a softmax over the classes at each of the ``L = prod(D)``
    positions): exact, ``S [C L, N, C, *D]`` with row ``v = c' L + l'`` and
    ``S[v, n, c, l] = [l = l'] sqrt(p[n, c', l]) ([c = c'] - p[n, c, l]) * scale``, or, with ``idx [M, N, *D]`` int32 class indices,
    the sampled factor ``S[m, n, c, l] = (p[n, c, l] - [c = idx[m, n, l]]) * scale`` (an index outside ``[0, C)`` matches no class).

    ``logits`` may be contiguous (class stride ``L``) or a permuted view of a contiguous ``[N, *D, C]`` (class stride 1); any other
    strides are copied first.  Every ``(v, n)`` slice of ``S`` has the memory format of a sample of ``logits``: for a permuted view,
    ``S.movedim(2, -1)`` is contiguous."""
    _require_device(logits)
    if logits.dim() < 3:
        raise ValueError(f"logits must be [N, C, *D] with at least one position dimension, got {tuple(logits.shape)}")
    N, C, D = logits.shape[0], logits.shape[1], tuple(logits.shape[2:])
    if C < 1:
        raise ValueError("logits must have at least one class")
    L = 1
    for d in D:
        L *= d
    if idx is not None:
        if idx.dtype != torch.int32:
            raise ValueError(f"idx must be int32 class indices, got {idx.dtype}")
        if idx.dim() != logits.dim() or tuple(idx.shape[1:]) != (N,) + D:
            raise ValueError(f"idx must be [M, {N}, {', '.join(map(str, D))}], got {tuple(idx.shape)}")
        if idx.device != logits.device:
            raise RuntimeError(f"all operands must live on one device (got {logits.device} and {idx.device})")
        idx = idx.contiguous()
    classes_last = logits.movedim(1, -1).is_contiguous()
    if not classes_last:
        logits = logits.contiguous()
    Vd = C * L if idx is None else idx.shape[0]
    if classes_last:
        S = torch.empty((Vd, N) + D + (C,), dtype=torch.float32, device=logits.device).movedim(-1, 2)
    else:
        S = torch.empty((Vd, N, C) + D, dtype=torch.float32, device=logits.device)
    st = _lib.load().vivit_ce_pos_sqrt_hessian_f32(logits.data_ptr(), idx.data_ptr() if idx is not None else None, S.data_ptr(), N, C, L, Vd,
                                                  1 if classes_last else 0, float(scale), _stream(logits))
    _lib.check(st, "vivit_ce_pos_sqrt_hessian_f32")
    return S


@_launcher
def ce_target_scales(target, num_classes: int, weight=None, ignore_index: int = -100, label_smoothing: float = 0.0, mean: bool = True,
                     mult: int = 1):
    """The scale of every position of a cross entropy with class-index targets, ``pos_scale`` (float32, the shape of ``target``), for
    :func:`ce_sqrt_hessian_positions_w` and :func:`ce_sqrt_hessian_w` (``vivit_ce_target_scales_f32``): with ``w`` the class weights
    (ones if absent) and ``a = (1 - eps) w[y] + eps mean(w)`` at a counted position (``y != ignore_index`` and ``0 <= y < C``), else 0,
    ``pos_scale = sqrt(a) / sqrt(mult norm)``, ``norm`` the sum of ``w[y]`` over the counted positions (``mean``) or 1.  ``target``
    int64 ``[N, *D]`` on the device; nothing comes back to the host."""
    if not target.is_cuda or target.dtype != torch.int64:
        raise RuntimeError(f"target must be an int64 tensor on a HIP device (got {target.dtype} on {target.device})")
    _require_device(weight)
    if weight is not None:
        if weight.device != target.device:
            raise RuntimeError(f"all operands must live on one device (got {target.device} and {weight.device})")
        if tuple(weight.shape) != (num_classes,):
            raise ValueError(f"weight must be [{num_classes}], got {tuple(weight.shape)}")
        weight = weight.contiguous()
    if mult < 1:
        raise ValueError(f"mult must be positive, got {mult}")
    target = target.contiguous()
    lib = _lib.load()
    R = target.numel()
    out = torch.empty(target.shape, dtype=torch.float32, device=target.device)
    ws, wsb = _workspace(lib.vivit_ce_target_scales_f32_workspace_bytes(R, num_classes), out)
    st = lib.vivit_ce_target_scales_f32(target.data_ptr(), weight.data_ptr() if weight is not None else None, out.data_ptr(), R, num_classes,
                                        int(ignore_index), float(label_smoothing), 1 if mean else 0, int(mult), ws, wsb, _stream(out))
    _lib.check(st, "vivit_ce_target_scales_f32")
    return out


@_launcher
def ce_sqrt_hessian_w(logits, row_scale, onehot=None):
    """:func:`ce_sqrt_hessian` with one scale per sample, ``row_scale [N]`` (``vivit_ce_sqrt_hessian_w_f32``): a sample whose scale is
    zero is exact zeros in every slice, whatever its logits hold."""
    _require_device(logits, onehot, row_scale)
    logits = logits.contiguous()
    N, C = logits.shape
    Vd = C if onehot is None else onehot.shape[0]
    if onehot is not None:
        onehot = onehot.contiguous()
        if tuple(onehot.shape[1:]) != (N, C):
            raise ValueError(f"onehot must be [M, {N}, {C}], got {tuple(onehot.shape)}")
    if row_scale.numel() != N:
        raise ValueError(f"row_scale must hold {N} floats, got {tuple(row_scale.shape)}")
    row_scale = row_scale.contiguous()
    S = torch.empty((Vd, N, C), dtype=torch.float32, device=logits.device)
    st = _lib.load().vivit_ce_sqrt_hessian_w_f32(logits.data_ptr(), onehot.data_ptr() if onehot is not None else None, row_scale.data_ptr(),
                                                S.data_ptr(), N, C, Vd, _stream(logits))
    _lib.check(st, "vivit_ce_sqrt_hessian_w_f32")
    return S


@_launcher
def ce_sqrt_hessian_positions_w(logits, pos_scale, idx=None):
    """:func:`ce_sqrt_hessian_positions` with one scale per position, ``pos_scale [N, *D]`` (``vivit_ce_pos_sqrt_hessian_w_f32``;
    ``sqrt(omega)`` for the exact factor, ``sqrt(omega / M)`` for the sampled one): a position whose scale is zero is exact zeros in
    every slice that covers it, whatever its logits hold.  Shapes, strides and the memory format of ``S`` as there."""
    _require_device(logits, pos_scale)
    if logits.dim() < 3:
        raise ValueError(f"logits must be [N, C, *D] with at least one position dimension, got {tuple(logits.shape)}")
    N, C, D = logits.shape[0], logits.shape[1], tuple(logits.shape[2:])
    if C < 1:
        raise ValueError("logits must have at least one class")
    L = 1
    for d in D:
        L *= d
    if tuple(pos_scale.shape) != (N,) + D:
        raise ValueError(f"pos_scale must be [{N}, {', '.join(map(str, D))}], got {tuple(pos_scale.shape)}")
    pos_scale = pos_scale.contiguous()
    if idx is not None:
        if idx.dtype != torch.int32:
            raise ValueError(f"idx must be int32 class indices, got {idx.dtype}")
        if idx.dim() != logits.dim() or tuple(idx.shape[1:]) != (N,) + D:
            raise ValueError(f"idx must be [M, {N}, {', '.join(map(str, D))}], got {tuple(idx.shape)}")
        if idx.device != logits.device:
            raise RuntimeError(f"all operands must live on one device (got {logits.device} and {idx.device})")
        idx = idx.contiguous()
    classes_last = logits.movedim(1, -1).is_contiguous()
    if not classes_last:
        logits = logits.contiguous()
    Vd = C * L if idx is None else idx.shape[0]
    if classes_last:
        S = torch.empty((Vd, N) + D + (C,), dtype=torch.float32, device=logits.device).movedim(-1, 2)
    else:
        S = torch.empty((Vd, N, C) + D, dtype=torch.float32, device=logits.device)
    st = _lib.load().vivit_ce_pos_sqrt_hessian_w_f32(logits.data_ptr(), idx.data_ptr() if idx is not None else None, pos_scale.data_ptr(),
                                                    S.data_ptr(), N, C, L, Vd, 1 if classes_last else 0, _stream(logits))
    _lib.check(st, "vivit_ce_pos_sqrt_hessian_w_f32")
    return S


@_launcher
def pack_lower(G: torch.Tensor) -> torch.Tensor:
    """Lower triangle (diagonal included) of the square matrix ``G`` as a packed ``n (n + 1) / 2`` vector (row-major)."""
    _require_device(G)
    G = _as2d(G)
    n = G.shape[0]
    packed = torch.empty(n * (n + 1) // 2, dtype=torch.float32, device=G.device)
    st = _lib.load().vivit_pack_lower_f32(G.data_ptr(), n, _ld(G), packed.data_ptr(), _stream(G))
    _lib.check(st, "vivit_pack_lower_f32")
    return packed


@_launcher
def unpack_lower_(packed: torch.Tensor, G: torch.Tensor) -> torch.Tensor:
    """Inverse of :func:`pack_lower` into the (row-major) ``G``, both triangles written (symmetric result)."""
    _require_device(packed, G)
    n = G.shape[0]
    if G.dim() != 2 or G.shape[1] != n or G.stride(1) != 1 or packed.numel() != n * (n + 1) // 2 or not packed.is_contiguous():
        raise ValueError("unpack_lower_ needs a square row-major G and a contiguous packed vector of n (n + 1) / 2 floats")
    st = _lib.load().vivit_unpack_lower_f32(packed.data_ptr(), n, G.data_ptr(), _ld(G), _stream(G))
    _lib.check(st, "vivit_unpack_lower_f32")
    return G


def _square_batch(mats, who: str):
    """``B`` square matrices of one size on one device, from a list or a ``[B, n, n]`` tensor, as a list (``who``: the calling
    function, named in the errors)."""
    mats = list(mats.unbind(0)) if isinstance(mats, torch.Tensor) and mats.dim() == 3 else list(mats)
    if not mats:
        raise ValueError(f"{who} needs at least one matrix")
    _require_device(*mats)
    for G in mats:
        if G.dim() != 2 or G.shape[0] != G.shape[1]:
            raise ValueError(f"Input must be a square matrix. Got shape {tuple(G.shape)}.")
        if G.shape != mats[0].shape:
            raise ValueError(f"{who} needs matrices of one size, got {tuple(mats[0].shape)} and {tuple(G.shape)}")
    return mats


def _batch_work(mats, n: int, overwrite: bool):
    """What a batched solver works on: every matrix with leading dimension ``n``, cloned unless it may be overwritten."""
    work = []
    for G in mats:
        A = _as2d(G)
        if _ld(A) != n:
            A = A.contiguous()   # one leading dimension for the whole batch
        if A.data_ptr() == G.data_ptr() and not overwrite:
            A = A.clone()  # the solver destroys its inputs
        work.append(A)
    return work


def _keep_indices(keep, n: int):
    """``keep`` (ints or an integer tensor, any order, repeats, negatives) as a list of positions in ``range(n)``."""
    keep = [int(k) for k in (keep.tolist() if isinstance(keep, torch.Tensor) else keep)]
    keep = [k + n if k < 0 else k for k in keep]
    if any(k < 0 or k >= n for k in keep):
        raise IndexError(f"eigenvector index out of range for n = {n}")
    return keep


def _rows_in_order(Zt, uniq, keep):
    """Rows of ``Zt`` (one per entry of ``uniq = sorted(set(keep))``) in the caller's order, repeats included."""
    if uniq == keep:
        return Zt
    pos = {k: i for i, k in enumerate(uniq)}
    return Zt[torch.tensor([pos[k] for k in keep], dtype=torch.long, device=Zt.device)]


class SymeigPlan:
    """A symmetric matrix reduced to tridiagonal form with ALL eigenvalues known (``evals``, ascending), waiting for
    the caller to say which eigenvectors it wants: the two launches around the reference's ``criterion`` callback
    (vivit/linalg/eigh.py:248-253).  :meth:`select` returns ``evecs[:, keep]`` of the reference."""

    def __init__(self, evals, n, A=None, state=None, full=None):
        self.evals, self.n = evals, n
        self._A, self._state, self._full = A, state, full

    @_launcher_method
    def select(self, keep) -> torch.Tensor:
        """``[n, K]`` column eigenvectors of ``evals[keep]`` (``keep``: any order, list of ints or an integer tensor)."""
        n = self.n
        dev = self.evals.device
        keep = _keep_indices(keep, n)
        K = len(keep)
        if self._full is not None:  # small problem: all vectors already there
            return self._full[:, keep]
        if K == 0:
            return torch.empty((n, 0), dtype=torch.float32, device=dev)
        uniq = sorted(set(keep))
        idx = torch.tensor(uniq, dtype=torch.int32, device=dev)
        Zt = torch.empty((len(uniq), n), dtype=torch.float32, device=dev)
        info = torch.zeros(1, dtype=torch.int32, device=dev)
        lib = _lib.load()
        ws, wsb = _workspace(lib.vivit_symeig_select_f32_workspace_bytes(n, len(uniq)), self.evals)
        st = lib.vivit_symeig_select_f32(
            self._A.data_ptr(), n, _ld(self._A), idx.data_ptr(), len(uniq), Zt.data_ptr(), n, self._state.data_ptr(),
            self._state.numel(), ws, wsb, info.data_ptr(), _stream(self.evals))
        _lib.check(st, "vivit_symeig_select_f32")
        check_info(info)
        return _rows_in_order(Zt, uniq, keep).T


@_launcher
def symeig_reduce(G: torch.Tensor, overwrite: bool = False) -> SymeigPlan:
    """Phase 1 of the selected-eigenvector solver: all eigenvalues of symmetric ``G`` (ascending, in ``plan.evals``)
    and a reduced state from which ``plan.select(keep)`` produces only the wanted eigenvectors
    (``vivit_symeig_reduce_f32`` / ``vivit_symeig_select_f32``).  Synchronises (the caller's criterion needs the
    eigenvalues anyway) and raises ``RuntimeError`` on non-convergence like :func:`symeig`."""
    _require_device(G)
    if G.dim() != 2 or G.shape[0] != G.shape[1]:
        raise ValueError(f"Input must be a square matrix. Got shape {tuple(G.shape)}.")
    n = G.shape[0]
    if n < SYMEIG_ROWS_MIN_N:  # single-workgroup solver: all vectors cost nothing extra
        w, Z = symeig(G, eigenvectors=True, overwrite=overwrite)
        return SymeigPlan(w, n, full=Z)
    lib = _lib.load()

    def solve():
        A = _as2d(G)
        if A.data_ptr() == G.data_ptr() and not overwrite:
            A = A.clone()
        w = torch.empty(n, dtype=torch.float32, device=G.device)
        info = torch.zeros(1, dtype=torch.int32, device=G.device)
        state = torch.empty(lib.vivit_symeig_reduce_f32_workspace_bytes(n) + 256, dtype=torch.uint8, device=G.device)
        st = lib.vivit_symeig_reduce_f32(A.data_ptr(), n, _ld(A), w.data_ptr(), state.data_ptr(), state.numel(),
                                         info.data_ptr(), _stream(G))
        _lib.check(st, "vivit_symeig_reduce_f32")
        check_info(info)
        return SymeigPlan(w, n, A=A, state=state)

    return _retry_on_launch_chain(solve, intact=not overwrite, G=G)


class PersistentKernelTimeout(RuntimeError):
    """A persistent kernel of the eigensolver (one-launch tridiagonalisation, panel QR, bulge chase) could not get its
    workgroups resident together -- twice -- or one of its exchanges stalled: ``info = VIVIT_INFO_PERSIST_TIMEOUT``
    (include/vivit_hip.h, "Persistent kernels").  Not a numerical failure: the input may be fine; something else held
    the GPU's compute units (another process on the card, a long collective).  The solve's outputs are garbage."""


def check_info(info: torch.Tensor):
    """Map the eigensolver's device-side status word to the reference's RuntimeError (synchronises);
    :class:`PersistentKernelTimeout` (a RuntimeError too) for the persistent kernels' own status."""
    nfail = int(info.item())
    if nfail == _lib.VIVIT_INFO_PERSIST_TIMEOUT:
        raise PersistentKernelTimeout(
            "symeig: a persistent kernel could not become resident (two attempts of 2 s) or stalled; "
            "VIVIT_SYTRD_PERSIST=0 VIVIT_QR_PERSIST=0 VIVIT_SB2ST_PERSIST=0 select the launch chains")
    if nfail != 0:
        raise RuntimeError(f"symeig: {nfail} eigenvalues did not converge")


class persistent_kernels:
    """``with persistent_kernels(False): ...`` -- run the enclosed solves on the launch chains
    (``vivit_persistent_kernels``; the previous setting is restored on exit)."""

    def __init__(self, on: bool):
        self._on = 1 if on else 0

    def __enter__(self):
        self._prev = _lib.load().vivit_persistent_kernels(self._on)
        return self

    def __exit__(self, *exc):
        _lib.load().vivit_persistent_kernels(self._prev)
        return False


_BACKUP_ALWAYS_BYTES = 256 << 20   # inputs up to this size (n <= 8192) are always backed up before an in-place solve


def _wants_backup(G: torch.Tensor) -> bool:
    """An in-place solve (``overwrite=True``) keeps a copy of its input for the launch-chain retry when that is cheap
    (<= 256 MB: 0.1 ms) or when the card is likely to be shared -- a multi-rank job, whose RCCL kernels compete with the
    persistent kernels for compute units -- or on request (``VIVIT_PERSIST_BACKUP=1``; ``=0`` never)."""
    import os

    env = os.environ.get("VIVIT_PERSIST_BACKUP")
    if env is not None:
        return env != "0"
    if G.numel() * 4 <= _BACKUP_ALWAYS_BYTES:
        return True
    import torch.distributed as dist

    return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1


def _retry_on_launch_chain(solve, intact: bool, G=None, what: str = "symeig"):
    """Run ``solve()``; if it ends with :class:`PersistentKernelTimeout` and the input is still there -- the solve worked
    on a copy (``intact``), or ``G`` (one matrix, or the list of a batch) is solved in place and was backed up
    (:func:`_wants_backup`, all of a batch or none) -- repeat it ONCE with the persistent kernels switched off: the same
    stages as launch chains, which need no co-residency.  Otherwise the error propagates (the input is gone)."""
    batch = isinstance(G, (list, tuple))
    Gs = list(G) if batch else ([] if G is None else [G])
    backups = [g.clone() for g in Gs] if (not intact and Gs and all(_wants_backup(g) for g in Gs)) else None
    try:
        return solve()
    except PersistentKernelTimeout:
        if not intact and backups is None:
            raise
        import warnings

        warnings.warn(f"{what}: persistent kernel timed out; repeating the {'batch' if batch else 'solve'} on the launch chains",
                      RuntimeWarning)
        if backups is not None:
            for g, b in zip(Gs, backups):
                g.copy_(b)
        with persistent_kernels(False):
            return solve()


SYMEIGVALS_BATCHED_MAX_N = 1280  # above: the whole chip per problem (vivit_symeigvals_batched_f32: VIVIT_E_UNSUPPORTED)


def check_info_batched(info: torch.Tensor, what: str = "symeigvals_batched"):
    """:func:`check_info` for the ``[B]`` status vector of a batched solve: ONE device->host read; the error names the
    failing problem."""
    host = info.tolist()
    for i, nfail in enumerate(host):
        if nfail == _lib.VIVIT_INFO_PERSIST_TIMEOUT:
            raise PersistentKernelTimeout(
                f"{what}: a persistent kernel could not become resident (two attempts of 2 s) or stalled "
                f"(reported at problem {i}; the whole batch is void); "
                "VIVIT_SYTRD_PERSIST=0 VIVIT_QR_PERSIST=0 VIVIT_SB2ST_PERSIST=0 select the launch chains")
    for i, nfail in enumerate(host):
        if nfail != 0:
            raise RuntimeError(f"{what}: problem {i}: {nfail} eigenvalues did not converge")


@_launcher
def symeigvals_batched(mats, overwrite: bool = False, info_out: Optional[list] = None) -> torch.Tensor:
    """Eigenvalues (ascending, row ``b`` = problem ``b``) of ``B`` symmetric matrices of ONE size: a list of ``[n, n]``
    tensors or a ``[B, n, n]`` tensor, fp32, on one device.  ``ValueError`` for mixed sizes.

    For 193 <= n <= 1280 eight problems share one launch of the persistent tridiagonalisation, one per XCD (a single
    ``symeig`` of that size occupies one XCD and idles seven); n <= 192 runs one workgroup per problem; n > 1280 is a loop
    over :func:`symeig`.  Every row equals ``symeig(G_b, eigenvectors=False)[0]`` bit for bit.

    Same contract as :func:`symeig`: the inputs are solved in place only with ``overwrite=True``; the ``[B]`` ``info``
    vector is read once (``RuntimeError`` names the failing problem) unless a list is passed as ``info_out``, which then
    receives it; a :class:`PersistentKernelTimeout` repeats the batch once on the launch chains when the inputs are
    still there (copies, or backed up: :func:`_wants_backup`)."""
    mats = _square_batch(mats, "symeigvals_batched")
    n, B, dev = mats[0].shape[0], len(mats), mats[0].device
    if n > SYMEIGVALS_BATCHED_MAX_N or n == 0:
        infos = [] if info_out is not None else None
        W = torch.stack([symeig(G, eigenvectors=False, overwrite=overwrite, info_out=infos)[0] for G in mats]) if n else \
            torch.empty((B, 0), dtype=torch.float32, device=dev)
        if info_out is not None:
            info_out.append(torch.cat(infos) if infos else torch.zeros(B, dtype=torch.int32, device=dev))
        return W
    lib = _lib.load()

    def solve():
        work = _batch_work(mats, n, overwrite)
        W = torch.empty((B, n), dtype=torch.float32, device=dev)
        info = torch.zeros(B, dtype=torch.int32, device=dev)
        ws, wsb = _workspace(lib.vivit_symeigvals_batched_f32_workspace_bytes(n, B), mats[0])
        ptrs = (ctypes.c_void_p * B)(*[A.data_ptr() for A in work])
        st = lib.vivit_symeigvals_batched_f32(ptrs, B, n, n, W.data_ptr(), ws, wsb, info.data_ptr(), _stream(mats[0]))
        _lib.check(st, "vivit_symeigvals_batched_f32")
        if info_out is not None:
            info_out.append(info)
        else:
            check_info_batched(info)
        return W

    return _retry_on_launch_chain(solve, intact=not overwrite, G=mats, what="symeigvals_batched")


class SymeigBatchPlan:
    """``B`` symmetric matrices of one size reduced together (:func:`symeig_reduce_batched`): ``evals`` is ``[B, n]``
    (row ``b`` ascending), ``plans[b]`` an ordinary :class:`SymeigPlan` of problem ``b`` that can still be selected from
    on its own, :meth:`select` the batched phase 2."""

    def __init__(self, evals, n, plans, work=None, state=None):
        self.evals, self.n, self.plans = evals, n, plans
        self._work, self._state = work, state

    @_launcher_method
    def select(self, keeps):
        """``keeps``: ``B`` index lists (rules of :meth:`SymeigPlan.select`: any order, repeats, negatives, ``IndexError``
        out of range; the lists may differ in length and may be empty).  Returns a list of ``[n, K_b]`` tensors."""
        n, B, dev = self.n, len(self.plans), self.evals.device
        keeps = [keep.tolist() if isinstance(keep, torch.Tensor) else list(keep) for keep in keeps]
        if len(keeps) != B:
            raise ValueError(f"need one index list per problem: got {len(keeps)} for {B} problems")
        keeps = [_keep_indices(keep, n) for keep in keeps]
        if self._state is None:  # sizes outside the batched range: problem after problem
            return [plan.select(keep) for plan, keep in zip(self.plans, keeps)]
        uniqs = [sorted(set(keep)) for keep in keeps]
        Ks = [len(u) for u in uniqs]
        if sum(Ks) == 0:
            return [torch.empty((n, 0), dtype=torch.float32, device=dev) for _ in keeps]
        idx = torch.tensor([k for u in uniqs for k in u], dtype=torch.int32, device=dev)
        Zt = torch.empty((sum(Ks), n), dtype=torch.float32, device=dev)
        rows = list(Zt.split(Ks))
        info = torch.zeros(B, dtype=torch.int32, device=dev)
        lib = _lib.load()
        ws, wsb = _workspace(lib.vivit_symeig_select_batched_f32_workspace_bytes(n, B, max(Ks)), self.evals)
        a_ptrs = (ctypes.c_void_p * B)(*[A.data_ptr() for A in self._work])
        z_ptrs = (ctypes.c_void_p * B)(*[(r.data_ptr() if K else None) for r, K in zip(rows, Ks)])
        s_ptrs = (ctypes.c_void_p * B)(*[s.data_ptr() for s in self._state])
        k_arr = (ctypes.c_int64 * B)(*Ks)
        st = lib.vivit_symeig_select_batched_f32(a_ptrs, B, n, n, idx.data_ptr(), k_arr, z_ptrs, n, s_ptrs,
                                                 self._state[0].numel(), ws, wsb, info.data_ptr(), _stream(self.evals))
        _lib.check(st, "vivit_symeig_select_batched_f32")
        check_info_batched(info, "symeig_reduce_batched.select")
        return [_rows_in_order(r, uniq, keep).T for r, uniq, keep in zip(rows, uniqs, keeps)]


@_launcher
def symeig_reduce_batched(mats, overwrite: bool = False, info_out: Optional[list] = None) -> SymeigBatchPlan:
    """Phase 1 of the selected-eigenvector solver for ``B`` symmetric matrices of ONE size (a list of ``[n, n]`` tensors or
    a ``[B, n, n]`` tensor, fp32, one device; ``ValueError`` for mixed sizes or an empty list): all eigenvalues in
    ``.evals`` ``[B, n]``, then ``.select(keeps)`` for only the wanted eigenvectors of every problem
    (``vivit_symeig_reduce_batched_f32`` / ``vivit_symeig_select_batched_f32``).

    For 193 <= n <= 1280 eight problems share one persistent tridiagonalisation launch (one per XCD), one bisection
    launch, and -- in ``select`` -- the inverse iteration and one back-transformation launch; row ``b`` of ``evals`` and
    ``plans[b].select(keep)`` equal ``symeig_reduce(G_b)`` bit for bit.  n < 193 and n > 1280 are loops over
    :func:`symeig_reduce`.  Contract of :func:`symeigvals_batched`: inputs solved in place only with ``overwrite=True``,
    one leading dimension per batch, ONE device->host read of the ``[B]`` ``info`` vector (``RuntimeError`` names the
    failing problem; a list passed as ``info_out`` receives the vector instead), and a
    :class:`PersistentKernelTimeout` repeats the batch once on the launch chains when the inputs are still there."""
    mats = _square_batch(mats, "symeig_reduce_batched")
    n, B, dev = mats[0].shape[0], len(mats), mats[0].device
    if n < SYMEIG_ROWS_MIN_N or n > SYMEIGVALS_BATCHED_MAX_N:
        plans = [symeig_reduce(G, overwrite=overwrite) for G in mats]
        if info_out is not None:
            info_out.append(torch.zeros(B, dtype=torch.int32, device=dev))
        return SymeigBatchPlan(torch.stack([p.evals for p in plans]), n, plans)
    lib = _lib.load()

    def solve():
        work = _batch_work(mats, n, overwrite)
        W = torch.empty((B, n), dtype=torch.float32, device=dev)
        info = torch.zeros(B, dtype=torch.int32, device=dev)
        each = (lib.vivit_symeig_reduce_f32_workspace_bytes(n) + 256 + 255) // 256 * 256
        state = list(torch.empty((B, each), dtype=torch.uint8, device=dev).unbind(0))
        a_ptrs = (ctypes.c_void_p * B)(*[A.data_ptr() for A in work])
        s_ptrs = (ctypes.c_void_p * B)(*[s.data_ptr() for s in state])
        st = lib.vivit_symeig_reduce_batched_f32(a_ptrs, B, n, n, W.data_ptr(), s_ptrs, each, info.data_ptr(), _stream(mats[0]))
        _lib.check(st, "vivit_symeig_reduce_batched_f32")
        if info_out is not None:
            info_out.append(info)
        else:
            check_info_batched(info, "symeig_reduce_batched")
        plans = [SymeigPlan(W[b], n, A=work[b], state=state[b]) for b in range(B)]
        return SymeigBatchPlan(W, n, plans, work=work, state=state)

    return _retry_on_launch_chain(solve, intact=not overwrite, G=mats, what="symeig_reduce_batched")


SYMEIG_ROWS_MIN_N = 193  # below: single-workgroup solver, no row-range entry point


@_launcher
def symeig_rows(G: torch.Tensor, row_begin: int, row_end: int, overwrite: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """All eigenvalues (ascending) of symmetric ``G`` and the eigenvectors ``row_begin .. row_end-1`` as ROWS
    ``[row_end - row_begin, n]`` (``vivit_symeig_rows_f32``): the unit of work of one rank in the multi-GPU
    eigensolver (``vivit_amd.distributed.symeig``)."""
    _require_device(G)
    if G.dim() != 2 or G.shape[0] != G.shape[1]:
        raise ValueError(f"Input must be a square matrix. Got shape {tuple(G.shape)}.")
    n = G.shape[0]
    if not (0 <= row_begin <= row_end <= n):
        raise ValueError(f"invalid eigenvector range [{row_begin}, {row_end}) for n = {n}")
    if n < SYMEIG_ROWS_MIN_N:  # same HIP solver, slice afterwards
        w, Z = symeig(G, eigenvectors=True, overwrite=overwrite)
        return w, Z.T[row_begin:row_end].contiguous()
    lib = _lib.load()

    def solve():
        A = _as2d(G)
        if A.data_ptr() == G.data_ptr() and not overwrite:
            A = A.clone()
        w = torch.empty(n, dtype=torch.float32, device=G.device)
        Zt = torch.empty((max(row_end - row_begin, 1), n), dtype=torch.float32, device=G.device)
        info = torch.zeros(1, dtype=torch.int32, device=G.device)
        ws, wsb = _workspace(lib.vivit_symeig_f32_workspace_bytes(n, 1), G)
        st = lib.vivit_symeig_rows_f32(
            A.data_ptr(), n, _ld(A), w.data_ptr(), Zt.data_ptr(), n, row_begin, row_end, ws, wsb, info.data_ptr(), _stream(G)
        )
        _lib.check(st, "vivit_symeig_rows_f32")
        check_info(info)
        return w, Zt[: row_end - row_begin]

    return _retry_on_launch_chain(solve, intact=not overwrite, G=G)


@_launcher
def stedc(d: torch.Tensor, e: torch.Tensor, eigenvectors: bool = False):
    """Eigen-decomposition of the symmetric tridiagonal (d, e) -- stage 2 of ``symeig`` (testing)."""
    _require_device(d, e)
    n = d.numel()
    d, e = d.contiguous().clone(), e.contiguous().clone()
    w = torch.empty(n, dtype=torch.float32, device=d.device)
    Z = torch.empty((n, n), dtype=torch.float32, device=d.device) if eigenvectors else None
    info = torch.zeros(1, dtype=torch.int32, device=d.device)
    lib = _lib.load()
    ws, wsb = _workspace(lib.vivit_stedc_f32_workspace_bytes(n, 1 if eigenvectors else 0), d)
    st = lib.vivit_stedc_f32(
        d.data_ptr(), e.data_ptr(), n, w.data_ptr(), Z.data_ptr() if eigenvectors else None, n, ws, wsb, info.data_ptr(), _stream(d)
    )
    _lib.check(st, "vivit_stedc_f32")
    if int(info.item()) != 0:
        raise RuntimeError(f"stedc: {int(info.item())} eigenvalues did not converge")
    return w, Z


@_launcher
def sytrd(G: torch.Tensor):
    """Householder tridiagonalisation -- stage 1 of ``symeig`` (testing).
    Returns ``(d, e, tau, A)`` with the reflectors in the upper triangle of ``A``."""
    _require_device(G)
    n = G.shape[0]
    A = G.contiguous().clone()
    d = torch.empty(n, dtype=torch.float32, device=G.device)
    e = torch.empty(n - 1, dtype=torch.float32, device=G.device)
    tau = torch.empty(n, dtype=torch.float32, device=G.device)
    lib = _lib.load()
    ws, wsb = _workspace(lib.vivit_sytrd_f32_workspace_bytes(n), G)
    st = lib.vivit_sytrd_f32(A.data_ptr(), n, n, d.data_ptr(), e.data_ptr(), tau.data_ptr(), ws, wsb, _stream(G))
    _lib.check(st, "vivit_sytrd_f32")
    return d, e, tau, A


@_launcher
def sy2sb(G: torch.Tensor):
    """Full symmetric -> band (testing). Returns ``(AB, tau1, A)``: band in row-band layout, reflector
    scalars, and the overwritten matrix (band + reflector rows)."""
    _require_device(G)
    lib = _lib.load()
    n = G.shape[0]
    nb = lib.vivit_sb2st_half_bandwidth()
    A = G.contiguous().clone()
    AB = torch.empty((n, 2 * nb + 1), dtype=torch.float32, device=G.device)
    tau1 = torch.empty(n, dtype=torch.float32, device=G.device)
    ws, wsb = _workspace(lib.vivit_sy2sb_f32_workspace_bytes(n), G)
    st = lib.vivit_sy2sb_f32(A.data_ptr(), n, n, AB.data_ptr(), tau1.data_ptr(), ws, wsb, _stream(G))
    _lib.check(st, "vivit_sy2sb_f32")
    return AB, tau1, A


BAND_NB = 64  # half bandwidth of the two-stage reduction (vivit_sb2st_half_bandwidth())


@_launcher
def symeig_prepare_(A: torch.Tensor) -> torch.Tensor:
    """In place: LAPACK-style scaling of symmetric ``A`` (lower triangle read) and mirror into the upper triangle --
    the state the band reduction starts from.  Returns the device ``scal[16]`` block for
    :func:`symeig_banded_rows` (``vivit_symeig_prepare_f32``)."""
    _require_device(A)
    n = A.shape[0]
    scal = torch.zeros(16, dtype=torch.float32, device=A.device)
    lib = _lib.load()
    ws, wsb = _workspace(8 * n + 512, A)
    st = lib.vivit_symeig_prepare_f32(A.data_ptr(), n, _ld(A), scal.data_ptr(), ws, wsb, _stream(A))
    _lib.check(st, "vivit_symeig_prepare_f32")
    return scal


@_launcher
def panel_qr_(pan: torch.Tensor):
    """Householder QR of one sub-band panel ``pan [mp, 64]`` (contiguous, factored in place: R's strict upper triangle
    stays in its first 64 rows).  Returns ``(Vt [64, mp], tau [64], betas [64], T [64, 64])`` with ``Q = I - V T V^T``
    (``vivit_sy2sb_panel_qr_f32``): the step every rank of the sharded band reduction repeats."""
    _require_device(pan)
    mp = pan.shape[0]
    if pan.dim() != 2 or pan.shape[1] != BAND_NB or not pan.is_contiguous():
        raise ValueError(f"panel must be a contiguous [mp, {BAND_NB}] matrix, got {tuple(pan.shape)}")
    dev = pan.device
    Vt = torch.empty((BAND_NB, mp), dtype=torch.float32, device=dev)
    tau = torch.empty(BAND_NB, dtype=torch.float32, device=dev)
    betas = torch.empty(BAND_NB, dtype=torch.float32, device=dev)
    T = torch.empty((BAND_NB, BAND_NB), dtype=torch.float32, device=dev)
    lib = _lib.load()
    ws, wsb = _workspace(lib.vivit_sy2sb_panel_qr_f32_workspace_bytes(mp), pan)
    st = lib.vivit_sy2sb_panel_qr_f32(pan.data_ptr(), mp, Vt.data_ptr(), mp, tau.data_ptr(), betas.data_ptr(), T.data_ptr(), ws,
                                      wsb, _stream(pan))
    _lib.check(st, "vivit_sy2sb_panel_qr_f32")
    return Vt, tau, betas, T


@_launcher
def symeig_banded_rows(A: torch.Tensor, tau1: torch.Tensor, scal: torch.Tensor, row_begin: int, row_end: int):
    """The two-stage solver entered after the band reduction (``A``: band + first-stage reflectors as ``sy2sb`` leaves
    them, destroyed): all eigenvalues and the eigenvectors ``row_begin .. row_end-1`` as rows
    (``vivit_symeig_banded_rows_f32``)."""
    _require_device(A)
    n = A.shape[0]
    w = torch.empty(n, dtype=torch.float32, device=A.device)
    Zt = torch.empty((max(row_end - row_begin, 1), n), dtype=torch.float32, device=A.device)
    info = torch.zeros(1, dtype=torch.int32, device=A.device)
    lib = _lib.load()
    ws, wsb = _workspace(lib.vivit_symeig_f32_workspace_bytes(n, 1), A)
    st = lib.vivit_symeig_banded_rows_f32(A.data_ptr(), n, _ld(A), tau1.data_ptr(), scal.data_ptr(), w.data_ptr(), Zt.data_ptr(),
                                          n, row_begin, row_end, ws, wsb, info.data_ptr(), _stream(A))
    _lib.check(st, "vivit_symeig_banded_rows_f32")
    check_info(info)
    return w, Zt[: row_end - row_begin]


@_launcher
def sb2st(AB: torch.Tensor):
    """Band -> tridiagonal by bulge chasing (testing). ``AB``: [n, 2*NB+1] row-band layout.
    Returns ``(d, e, R2, tau2)``."""
    _require_device(AB)
    lib = _lib.load()
    n = AB.shape[0]
    nb = lib.vivit_sb2st_half_bandwidth()
    assert AB.shape[1] == 2 * nb + 1 and AB.is_contiguous()
    AB = AB.clone()
    d = torch.empty(n, dtype=torch.float32, device=AB.device)
    e = torch.empty(n, dtype=torch.float32, device=AB.device)
    R2 = torch.zeros((n, n), dtype=torch.float32, device=AB.device)
    nbytes = lib.vivit_sb2st_f32_workspace_bytes(n)
    ws = torch.zeros(nbytes + 256, dtype=torch.uint8, device=AB.device)
    st = lib.vivit_sb2st_f32(AB.data_ptr(), n, d.data_ptr(), e.data_ptr(), R2.data_ptr(), ws.data_ptr(), ws.numel(), _stream(AB))
    _lib.check(st, "vivit_sb2st_f32")
    off = (-ws.data_ptr()) % 256
    nk = -(-n // nb) + 1
    tau2 = ws[off : off + 4 * n * nk].view(torch.float32).view(n, nk).clone()
    return d, e[: n - 1], R2, tau2


@_launcher
def q2_apply_(Zt: torch.Tensor, R2: torch.Tensor, tau2: torch.Tensor, mode: int = -1) -> torch.Tensor:
    """``Zt <- Zt Q2^T`` in place (testing): the back-transformation through the bulge-chasing reflectors ``(R2, tau2)``
    of :func:`sb2st`.  ``mode``: 0 block steps (fp32 MFMA), 1 sliding window on the bf16 pipe, -1 the solver's choice."""
    _require_device(Zt, R2, tau2)
    n = R2.shape[0]
    assert Zt.dim() == 2 and Zt.shape[1] == n and Zt.stride(1) == 1 and R2.is_contiguous() and tau2.is_contiguous()
    lib = _lib.load()
    nbytes = lib.vivit_q2_apply_f32_workspace_bytes(n)
    ws, wsb = _workspace(nbytes, Zt)
    st = lib.vivit_q2_apply_f32(Zt.data_ptr(), Zt.stride(0), Zt.shape[0], n, R2.data_ptr(), n, tau2.data_ptr(), ws, wsb, int(mode),
                                _stream(Zt))
    _lib.check(st, "vivit_q2_apply_f32")
    return Zt


@_launcher
def dir_curvature(GE, evals, C: int, N: int, scale: float):
    """``lambdas[n,k] = scale * sum_c GE[(c,n),k]^2 / evals[k]`` (K6 epilogue)."""
    _require_device(GE, evals)
    GE, evals = GE.contiguous(), evals.contiguous()
    K = evals.numel()
    out = torch.empty((N, K), dtype=torch.float32, device=GE.device)
    st = _lib.load().vivit_dir_curvature_f32(GE.data_ptr(), evals.data_ptr(), out.data_ptr(), C, N, K, scale, _stream(GE))
    _lib.check(st, "vivit_dir_curvature_f32")
    return out


@_launcher
def scale_cols_rsqrt_(X, evals, pre: float = 1.0):
    """In place ``X[:, k] *= pre / sqrt(evals[k])`` (K5 epilogue)."""
    _require_device(X, evals)
    if X.stride(1) != 1:
        raise ValueError("X must have unit column stride")
    rows, K = X.shape
    st = _lib.load().vivit_scale_cols_rsqrt_f32(X.data_ptr(), evals.contiguous().data_ptr(), rows, K, _ld(X), pre, _stream(X))
    _lib.check(st, "vivit_scale_cols_rsqrt_f32")
    return X


def _one_ld(mats, cols):
    """``mats`` as 2-d kernel operands that share ONE leading dimension: as they are when their strides agree,
    contiguous copies otherwise."""
    mats = [_as2d(t) for t in mats]
    lds = {_ld(t) for t in mats if t.shape[0] > 1}
    if len(lds) > 1:
        mats = [t.contiguous() for t in mats]
        lds = {max(cols, 1)}
    return mats, (lds.pop() if lds else max(cols, 1))


@_launcher
def gram_directions_batched(grams, Zts, evals, VtGs, C: int, N: int, alpha_gram: float, alpha_gamma: float,
                            lambda_scale: float):
    """K5 + K6 of ``B`` groups of one Gram size in ONE launch (``vivit_gram_directions_batched_f32``), ``G E`` never
    stored.  Per problem ``b``: ``grams[b] [n, n]`` (symmetric, ``n = C N``, left intact), ``Zts[b] [K_b, n]`` (rows = kept
    unit eigenvectors, i.e. ``evecs.T``; ``K_b`` may differ and may be 0), ``evals[b] [K_b]`` (kept eigenvalues, already
    scaled), ``VtGs[b] [n, M]``.  Returns ``(gammas, lambdas)``, two lists with

      ``gammas[b][j, k]  = alpha_gamma * sum_i VtGs[b][i, j] Zts[b][k, i] / sqrt(evals[b][k])``            ``[M, K_b]``
      ``lambdas[b][m, k] = lambda_scale * sum_c (alpha_gram * sum_i grams[b][(c, m), i] Zts[b][k, i])^2 / evals[b][k]``  ``[N, K_b]``

    ``ValueError`` for mixed ``n`` or ``M``, for list lengths that differ and for an empty batch."""
    grams, Zts, evals, VtGs = list(grams), list(Zts), list(evals), list(VtGs)
    B = len(grams)
    if B == 0:
        raise ValueError("gram_directions_batched needs at least one problem")
    if not (len(Zts) == len(evals) == len(VtGs) == B):
        raise ValueError(f"need one entry per problem in every list: got {B}, {len(Zts)}, {len(evals)}, {len(VtGs)}")
    _require_device(*grams, *Zts, *evals, *VtGs)
    n, dev = C * N, grams[0].device
    for G in grams:
        if G.dim() != 2 or G.shape[0] != G.shape[1]:
            raise ValueError(f"Input must be a square matrix. Got shape {tuple(G.shape)}.")
        if G.shape[0] != n:
            raise ValueError(f"gram_directions_batched needs Gram matrices of one size n = C N = {n}, got {tuple(G.shape)}")
    if any(V.dim() != 2 or V.shape[0] != n for V in VtGs):
        raise ValueError(f"every V^T g must be [{n}, M]")
    M = VtGs[0].shape[1]
    if any(V.shape[1] != M for V in VtGs):
        raise ValueError(f"gram_directions_batched needs one M, got {sorted({V.shape[1] for V in VtGs})}")
    Ks = [int(w.numel()) for w in evals]
    for Zt, K in zip(Zts, Ks):
        if Zt.dim() != 2 or tuple(Zt.shape) != (K, n):
            raise ValueError(f"Zt must be [K, n] = [{K}, {n}] (one row per kept eigenvalue), got {tuple(Zt.shape)}")
    grams, ldg = _one_ld(grams, n)
    VtGs, ldv = _one_ld(VtGs, M)
    Zts, ldz = _one_ld(Zts, n)
    evals = [w.contiguous() for w in evals]
    gam = torch.empty(M * sum(Ks), dtype=torch.float32, device=dev)
    lam = torch.empty(N * sum(Ks), dtype=torch.float32, device=dev)
    gammas = [g.view(M, K) for g, K in zip(gam.split([M * K for K in Ks]), Ks)]
    lambdas = [l.view(N, K) for l, K in zip(lam.split([N * K for K in Ks]), Ks)]

    def ptrs(ts):
        return (ctypes.c_void_p * B)(*[(t.data_ptr() if t.numel() else None) for t in ts])

    st = _lib.load().vivit_gram_directions_batched_f32(
        ptrs(grams), B, n, ldg, ptrs(Zts), ldz, ptrs(evals), ptrs(VtGs), ldv, (ctypes.c_int64 * B)(*Ks), C, N, M,
        alpha_gram, alpha_gamma, lambda_scale, ptrs(gammas), ptrs(lambdas), _stream(grams[0]))
    _lib.check(st, "vivit_gram_directions_batched_f32")
    return gammas, lambdas


@_launcher
def normalize_rows_(tensors):
    """Normalise ``K`` stacked vectors given in parameter-list format, in place (K10).

    ``tensors``: list of ``[K, *param.shape]`` contiguous tensors; afterwards, for each ``k``,
    ``sum_t ||tensors[t][k]||^2 == 1``.  Replaces vivit/linalg/utils.py:67-76.
    """
    if len(tensors) == 0:
        return tensors
    _require_device(*tensors)
    K = tensors[0].shape[0]
    lib = _lib.load()
    acc = torch.zeros(K, dtype=torch.float32, device=tensors[0].device)
    flat = []
    for t in tensors:
        if not t.is_contiguous():
            raise ValueError("normalize_rows_ needs contiguous tensors")
        length = t.numel() // max(K, 1)
        flat.append((t, length))
        ws, wsb = _workspace(lib.vivit_row_sqnorm_workspace_bytes(K, length), t)
        st = lib.vivit_row_sqnorm_acc_f32(t.data_ptr(), acc.data_ptr(), K, length, ws, wsb, _stream(t))
        _lib.check(st, "vivit_row_sqnorm_acc_f32")
    for t, length in flat:
        st = lib.vivit_scale_rows_rsqrt_f32(t.data_ptr(), acc.data_ptr(), K, length, _stream(t))
        _lib.check(st, "vivit_scale_rows_rsqrt_f32")
    return tensors
