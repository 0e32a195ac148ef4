"""Dense bf16 GEMM on the in-tree MFMA kernel (csrc/gemm_bf16.hip):

    C = alpha * op(A) * op(B) + bias + beta * C        (fp32 accumulation, fp32 or bf16 result)

in three operand forms over row-major operands whose inner dimension is contiguous:
    NT  (trans_b)            a [M, K], b [N, K]    forward x W^T
    NN                       a [M, K], b [K, N]    data gradient gy W (no transposed weight copy)
    TN  (trans_a)            a [P, M], b [P, N]    weight gradient gy^T x, optional colsum[M] += colscale * sum_p a[p]

Rules on the GPU (a breach raises ValueError; there is no fallback to a vendor library): every inner extent and
every leading dimension is a multiple of 8 elements, bases are 16-byte aligned, ``beta`` needs an fp32 ``out``,
``bias`` goes with NT / NN and ``colsum`` with TN. Row-strided views are taken as they are. CPU tensors compute
the same expression with torch in fp32 (the semantics the CPU test tier pins).

``backend()`` / ``set_backend("blas" | "native")`` choose who runs the language-model-scale plain GEMMs that
nn.Linear and the whole-sequence LSTM / GRU weight gradients send to hipBLASLt by default: ``native`` keeps them
on this kernel. Initialised from BIGDL_GEMM_BACKEND; Engine.setProperty("bigdl.gemm.backend", ...) sets it too.
"""
import os

import torch

from . import native

BF16 = torch.bfloat16
_BACKENDS = ("blas", "native")


def _checked(name):
    name = str(name).lower()
    if name not in _BACKENDS:
        raise ValueError(f"bigdl.gemm.backend must be one of {_BACKENDS}, got {name!r}")
    return name


_BACKEND = [_checked(os.environ.get("BIGDL_GEMM_BACKEND", "blas"))]


def backend():
    return _BACKEND[0]


def set_backend(name):
    _BACKEND[0] = _checked(name)


def _mat(t, name):
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[0] == 0 or t.shape[1] == 0:
        raise ValueError(f"gemm: {name} must be a non-empty matrix")
    if t.dtype not in (torch.float32, BF16):
        raise ValueError(f"gemm: {name} must be fp32 or bf16, got {t.dtype}")
    return t


def _rules(t, name):
    """The kernel's alignment rules for one 2-D operand (after any conversion)."""
    if t.stride(1) != 1:
        raise ValueError(f"gemm: the inner dimension of {name} must be contiguous")
    if t.shape[1] % 8:
        raise ValueError(f"gemm: the inner extent of {name} ({t.shape[1]}) must be a multiple of 8 elements")
    if t.shape[0] > 1 and (t.stride(0) % 8 or t.stride(0) < t.shape[1]):
        raise ValueError(f"gemm: the leading dimension of {name} ({t.stride(0)}) must be a multiple of 8 elements")
    if t.is_cuda and t.data_ptr() % 16:
        raise ValueError(f"gemm: {name} must be 16-byte aligned")


def _bf16_operand(t):
    if t.dtype == BF16:
        return t if t.stride(1) == 1 else t.contiguous()
    if t.is_cuda:
        from . import to_bf16

        return to_bf16(t)
    return t.to(BF16)


def gemm(a, b, *, trans_a=False, trans_b=False, out=None, out_dtype=torch.float32, alpha=1.0, beta=0.0, bias=None,
         colsum=None, colscale=1.0):
    """C = alpha * op(a) * op(b) + bias + beta * C; returns C (``out`` when given)."""
    if trans_a and trans_b:
        raise ValueError("gemm: the TT form (trans_a and trans_b) is not provided")
    form = 2 if trans_a else (0 if trans_b else 1)
    a, b = _mat(a, "a"), _mat(b, "b")
    M, K = (a.shape[1], a.shape[0]) if trans_a else (a.shape[0], a.shape[1])
    N, Kb = (b.shape[0], b.shape[1]) if trans_b else (b.shape[1], b.shape[0])
    if K != Kb:
        raise ValueError(f"gemm: reduction lengths differ ({K} vs {Kb})")
    if out is not None:
        if out.dim() != 2 or tuple(out.shape) != (M, N):
            raise ValueError(f"gemm: out must be [{M}, {N}]")
        out_dtype = out.dtype
    if out_dtype not in (torch.float32, BF16):
        raise ValueError("gemm: the result is fp32 or bf16")
    if beta != 0.0 and out_dtype != torch.float32:
        raise ValueError("gemm: beta needs an fp32 out")
    if beta != 0.0 and out is None:
        raise ValueError("gemm: beta needs an out to accumulate into")
    if bias is not None and form == 2:
        raise ValueError("gemm: bias goes with the NT / NN forms")
    if bias is not None and (bias.dim() != 1 or bias.shape[0] != N):
        raise ValueError(f"gemm: bias must be a vector of {N}")
    if colsum is not None and form != 2:
        raise ValueError("gemm: colsum goes with the TN form")
    if colsum is not None and (colsum.dim() != 1 or colsum.shape[0] != M or colsum.dtype != torch.float32
                               or not colsum.is_contiguous()):
        raise ValueError(f"gemm: colsum must be a dense fp32 vector of {M}")
    a16, b16 = _bf16_operand(a), _bf16_operand(b)
    _rules(a16, "a")
    _rules(b16, "b")
    if out is not None:
        _rules(out, "out")
    elif N % 8:
        raise ValueError(f"gemm: the inner extent of the result ({N}) must be a multiple of 8 elements")

    if not a.is_cuda:
        af = a16.float().t() if trans_a else a16.float()
        bf = b16.float().t() if trans_b else b16.float()
        c = alpha * (af @ bf)
        if bias is not None:
            c = c + bias.float()
        if beta != 0.0:
            c = c + beta * out
        if colsum is not None:
            colsum.add_(a16.float().sum(0), alpha=colscale)
        if out is None:
            return c.to(out_dtype)
        out.copy_(c)
        return out

    C = native.get()
    if out is None:
        out = torch.empty(M, N, dtype=out_dtype, device=a.device)
    if bias is not None:
        if bias.dtype not in (torch.float32, BF16):
            raise ValueError("gemm: bias must be fp32 or bf16")
        bias = bias.contiguous()
        if bias.data_ptr() % 16:
            raise ValueError("gemm: bias must be 16-byte aligned")
    nbytes = C.gemm_bf16_ws_bytes(form, M, N, K)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=a.device) if nbytes else None
    C.gemm_bf16(a16, b16, out, form, float(alpha), float(beta), bias, colsum, float(colscale), ws)
    return out
