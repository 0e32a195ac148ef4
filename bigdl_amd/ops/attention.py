"""Scaled-dot-product attention core: softmax(q k^T + bias) v over [B, heads, L, depth] tensors.

Reference: the MM(transB) -> CAddTable(bias) -> SoftMax -> Dropout -> MM chain of S/nn/Attention.scala:90-103.
GPU engine: the fused flash kernel (ops/flash_attention.py -> csrc/attention.hip) for head dims 32 / 64 / 96 / 128,
attention dropout included (in-kernel counter-hash mask, regenerated in the backward).
Math path (CPU engine, other head dims): explicit GEMMs + softmax under autograd
(q is pre-scaled by depth^-0.5 as in SplitHeads(mul=true), Attention.scala:256-275).

Single-token decoding over a preallocated KV cache (``decode_attention``, ``kv_append``, ``kv_reorder``):
csrc/attn_decode.hip on the GPU engine, torch elsewhere.
"""
import os

import torch

from . import native


def _flash_ok(q, k, v, bias, dropout_p):
    """The fused kernel (csrc/attention.hip) covers head dims 32 / 64 / 96 / 128 (with or without attention
    dropout); a bias that needs a gradient (anything but a constant mask) keeps the math path."""
    if not q.is_cuda or not (0.0 <= dropout_p < 1.0):
        return False
    if bias is not None and bias.requires_grad and not getattr(bias, "_bigdl_mask", True):
        return False
    d = q.shape[-1]
    return d in (32, 64, 96, 128) and q.shape[-2] >= 1 and k.shape[-2] >= 1 and (bias is None or bias.dim() <= 4)


def attention_math(q, k, v, bias=None, dropout_p=0.0, training=False):
    s = torch.matmul(q, k.transpose(-1, -2))
    if bias is not None:
        s = s + bias
    p = torch.softmax(s, dim=-1)
    if training and dropout_p > 0.0:
        p = torch.nn.functional.dropout(p, dropout_p, True)
    return torch.matmul(p, v)


# ---------------------------------------------------------------------------------------------- decoding
_DECODE_DIMS = (32, 64, 96, 128)
# Native incremental decoding of Transformer beam search (nn/transformer.py _DecodeState): BIGDL_DECODE_NATIVE /
# Engine property bigdl.decode.native; unset means the engine's default below (the CPU engine's is off)
_DECODE_NATIVE = [None]
DECODE_NATIVE_GPU_DEFAULT = True


def set_decode_native(v):
    """True / False, "1" / "0", or None for the engine's default."""
    _DECODE_NATIVE[0] = None if v is None or v == "" else str(v).lower() in ("1", "true", "yes")


def decode_native(is_cuda):
    v = _DECODE_NATIVE[0]
    if v is None:
        env = os.environ.get("BIGDL_DECODE_NATIVE", "")
        v = (is_cuda and DECODE_NATIVE_GPU_DEFAULT) if env == "" else env.lower() in ("1", "true", "yes")
    return bool(v)


def decode_cache_dtype(is_cuda, hidden, heads):
    """bf16 where the decode kernels run (GPU engine, supported head dim), else fp32: the math path then computes
    what the Table path computes."""
    return torch.bfloat16 if is_cuda and hidden % heads == 0 and hidden // heads in _DECODE_DIMS else torch.float32


def _decode_kernel_ok(q, kcache, heads):
    return q.is_cuda and kcache.dtype == torch.bfloat16 and q.shape[1] % heads == 0 and \
        q.shape[1] // heads in _DECODE_DIMS


def decode_attention_math(q, kcache, vcache, length, heads, rows=None, bias=None):
    N, hidden = q.shape
    D = hidden // heads
    k, v = kcache[:, :length], vcache[:, :length]
    b = None if bias is None else bias[:, :length]
    if rows is not None:
        ix = rows.long()
        k, v = k.index_select(0, ix), v.index_select(0, ix)
        b = None if b is None else b.index_select(0, ix)
    if kcache.dtype == torch.bfloat16:               # the kernel's operands: q rounded like the cache
        q = q.bfloat16()
    qh = q.float().view(N, 1, heads, D).transpose(1, 2)
    kh = k.float().view(N, length, heads, D).transpose(1, 2)
    vh = v.float().view(N, length, heads, D).transpose(1, 2)
    o = attention_math(qh, kh, vh, None if b is None else b.float().view(N, 1, 1, length))
    return o.transpose(1, 2).reshape(N, hidden)


def decode_attention(q, kcache, vcache, length, heads, rows=None, bias=None):
    """One query row per (sequence, head) over a preallocated cache: q [N, heads * D] fp32 (already scaled),
    kcache / vcache [R, Lmax, heads * D] of which positions 0 .. length - 1 are valid, rows (optional, int32 [N])
    the cache row of sequence n, bias (optional) fp32 [R, Lmax] read through the same rows. Returns o fp32
    [N, heads * D], heads combined.

    GPU engine, bf16 caches, head dims 32 / 64 / 96 / 128: csrc/attn_decode.hip. Otherwise (CPU engine, fp32
    caches, other head dims) the torch math of the same signature."""
    if _decode_kernel_ok(q, kcache, heads):
        q = q.float().contiguous()
        o = torch.empty_like(q)
        native.get().attn_decode(q, kcache, vcache, int(length), int(heads), rows, bias, o)
        return o
    return decode_attention_math(q, kcache, vcache, length, heads, rows, bias)


def kv_append(k, v, kcache, vcache, pos):
    """Write this step's K / V rows [N, hidden] into position ``pos`` of both caches [N, Lmax, hidden]."""
    if k.is_cuda and kcache.dtype == torch.bfloat16 and k.shape[1] % 8 == 0:
        native.get().kv_append(k.float().contiguous(), v.float().contiguous(), kcache, vcache, int(pos))
    else:
        kcache[:, pos] = k.to(kcache.dtype)
        vcache[:, pos] = v.to(vcache.dtype)


def kv_reorder(src, dst, parent, length):
    """dst[..., n, :length, :] = src[..., parent[n], :length, :] over [..., N, Lmax, hidden] buffers (never in
    place); parent int32 [N]."""
    if src.is_cuda and src.dtype == torch.bfloat16 and src.shape[-1] % 8 == 0:
        native.get().kv_reorder(src, dst, parent, int(length))
    else:
        assert src.data_ptr() != dst.data_ptr(), "kv_reorder is never in place"
        dst[..., :length, :] = src.index_select(-3, parent.long())[..., :length, :]


def attention(q, k, v, bias=None, dropout_p=0.0, training=False, causal=False):
    """q: [B, H, Lq, D] (already scaled), k/v: [B, H, Lk, D], bias broadcastable to [B, H, Lq, Lk].

    ``causal`` is a hint that ``bias`` is the lower-triangular -1e9 mask (Transformer SelfAttentionMask), which
    lets the fused kernel skip fully-masked key blocks.
    """
    p = dropout_p if training else 0.0
    if _flash_ok(q, k, v, bias, p):
        from .flash_attention import flash_attention

        seed = 0
        if p > 0.0:
            from .nnk import next_seed

            seed = next_seed()
        return flash_attention(q, k, v, None if causal else bias, causal, p, seed)
    return attention_math(q, k, v, bias, dropout_p, training)
