"""Sparse (COO) ops of the wide half of Wide & Deep models: SparseLinear, LookupTableSparse, SparseJoinTable.

Reference: S/nn/SparseLinear.scala (SparseTensorMath.addmm), S/nn/LookupTableSparse.scala,
S/nn/SparseJoinTable.scala (Tensor.sparseConcat).

Every function takes a 2-D ``torch.sparse_coo`` tensor (coalesced by torch first when it is not) and has two forms:

* the native form on the kernels of csrc/sparse.hip: the index lists are read as torch stores them, nothing is
  sized by B * D, nothing waits on the host;
* the torch form (``torch.sparse.mm``, ``to_dense`` / ``to_sparse``): what the CPU engine runs, and the GPU engine
  with the switch off.

Switch: BIGDL_SPARSE_NATIVE / Engine property bigdl.sparse.native / ``set_native``; unset means the engine's default
below (the CPU engine's is off). ``last_route()`` reports the form the last call took: "native", "ordered" (the
deterministic-mode form of the two weight gradients: stable sort, in-order sums, plain stores) or "torch". A weight
that is not fp32 on the GPU, or a join of more than 8 inputs, takes the torch form.
"""
import os

import torch

from . import native

_NATIVE = [None]
# tools/bench_sparse.py, profiles/sparse_native_ab.txt: the rule is native by default where its gain exceeds three
# times the larger round-to-round spread
NATIVE_GPU_DEFAULT = True
MAX_JOIN = 8
COMBINERS = {"sum": 0, "mean": 1, "sqrtn": 2}
_OPS = ("spmm", "spmm_wgrad", "sddmm", "lookup_sparse", "lookup_sparse_backward", "concat_cols")
_ROUTE = dict.fromkeys(_OPS + ("last",))


def set_native(v):
    """True / False, "1" / "0", or None for the engine's default."""
    _NATIVE[0] = None if v is None or v == "" else str(v).lower() in ("1", "true", "yes")


def native_on(is_cuda):
    v = _NATIVE[0]
    if v is None:
        env = os.environ.get("BIGDL_SPARSE_NATIVE", "")
        v = NATIVE_GPU_DEFAULT if env == "" else env.lower() in ("1", "true", "yes")
    return bool(v) and bool(is_cuda)


def last_route(op=None):
    """"native", "ordered" or "torch": the form the last call of ``op`` (one of this module's functions, by name)
    took; without ``op``, of whichever ran last."""
    return _ROUTE["last" if op is None else op]


def _set_route(op, route):
    _ROUTE[op] = _ROUTE["last"] = route


def _f32_gpu(*ts):
    return all(t is not None and t.is_cuda and t.dtype == torch.float32 for t in ts)


def _is_coo(x):
    return isinstance(x, torch.Tensor) and x.layout == torch.sparse_coo and x.dim() == 2 and x.dense_dim() == 0


class Coo:
    """Index list, fp32 values and (native form) CSR row offsets of a coalesced 2-D sparse tensor; build it once per
    tensor and hand it to every op of a forward / backward pair."""

    def __init__(self, x):
        src = x
        if not _is_coo(x):
            raise ValueError("ops.sparse: a 2-D sparse COO tensor is expected")
        if not x.is_coalesced():
            x = x.coalesce()
        self.src = src
        self.x = x
        self.shape = tuple(x.shape)
        self.idx = x._indices().contiguous()
        v = x._values()
        self.vals = (v if v.dtype == torch.float32 else v.float()).contiguous()
        self.nnz = self.idx.shape[1]
        self._offs = None

    @property
    def offs(self):
        if self._offs is None:
            self._offs = torch.empty(self.shape[0] + 1, dtype=torch.int32, device=self.idx.device)
            if self.nnz:
                native.get().coo_row_offsets(self.idx, self._offs)
            else:
                self._offs.zero_()
        return self._offs

    def x_as(self, dtype):
        return self.x if self.x.dtype == dtype else self.x.to(dtype)

    def with_values(self, vals):
        return torch.sparse_coo_tensor(self.idx, vals, self.shape, is_coalesced=True)


def coo(x):
    return x if isinstance(x, Coo) else Coo(x)


# ------------------------------------------------------------------------------------------------- SparseLinear
def spmm(x, weight, bias=None):
    """y [B, N] = x [B, D] (sparse) @ weight[N, D]^T + bias."""
    c = coo(x)
    if native_on(c.idx.is_cuda) and _f32_gpu(weight) and (bias is None or _f32_gpu(bias)):
        _set_route("spmm", "native")
        B, N = c.shape[0], weight.shape[0]
        if c.nnz == 0:
            y = torch.zeros(B, N, dtype=torch.float32, device=weight.device)
            return y if bias is None else y.add_(bias)
        y = torch.empty(B, N, dtype=torch.float32, device=weight.device)
        native.get().spmm_fwd(c.idx, c.vals, c.offs, weight.contiguous(), None if bias is None else bias.contiguous(), y)
        return y
    _set_route("spmm", "torch")
    y = torch.sparse.mm(c.x_as(weight.dtype), weight.t())
    return y + bias if bias is not None else y


def spmm_wgrad(x, gy, gradWeight, scale=1.0):
    """gradWeight [N, D] += scale * gy[B, N]^T @ x [B, D], in place; only the columns that occur are touched on the
    native form."""
    c = coo(x)
    if (native_on(c.idx.is_cuda) and _f32_gpu(gy, gradWeight) and gradWeight.is_contiguous()):
        if c.nnz == 0 or scale == 0:
            _set_route("spmm_wgrad", "ordered" if native.deterministic() else "native")
            return gradWeight
        r = native.get().spmm_wgrad(c.idx, c.vals, gy.contiguous(), gradWeight, float(scale))
        _set_route("spmm_wgrad", "ordered" if r else "native")
        return gradWeight
    _set_route("spmm_wgrad", "torch")
    g = torch.sparse.mm(c.x_as(gradWeight.dtype).t(), gy.to(gradWeight.dtype))          # dense [D, N]
    gradWeight.add_(g.t().to(gradWeight.dtype), alpha=scale)
    return gradWeight


def sddmm(x, gy, weight):
    """Values [nnz] of d loss / d x on x's own pattern: g_k = gy[row_k, :] . weight[:, col_k]."""
    c = coo(x)
    if native_on(c.idx.is_cuda) and _f32_gpu(gy, weight):
        _set_route("sddmm", "native")
        g = torch.empty(c.nnz, dtype=torch.float32, device=gy.device)
        if c.nnz:
            native.get().sddmm_rows(c.idx, gy.contiguous(), weight.contiguous(), g)
        return g
    _set_route("sddmm", "torch")
    rows, cols = c.idx[0], c.idx[1]
    return (gy.to(weight.dtype)[rows] * weight.t()[cols]).sum(1)


# ------------------------------------------------------------------------------------------------- LookupTableSparse
def _dense_ids(ids, weights, nIndex, dtype):
    """Today's dense view of the id / weight pair: 0-based rows [B, L] (clamped), per-slot weight (0 where there is no
    in-range id)."""
    dense = ids.x.to_dense() if isinstance(ids, Coo) else ids
    idx = dense.long() - 1
    mask = ((idx >= 0) & (idx < nIndex)).to(dtype)
    if weights is None:
        w = mask
    else:
        wd = weights.x.to_dense() if isinstance(weights, Coo) else weights
        w = wd.to(dtype) * mask
    return idx.clamp(0, max(nIndex - 1, 0)), w


def _row_scale(w, combiner):
    if combiner == "mean":
        den = w.sum(1)
        return torch.where(den != 0, 1.0 / den, torch.zeros_like(den))
    if combiner == "sqrtn":
        den = (w * w).sum(1)
        return torch.where(den > 0, den.rsqrt(), torch.zeros_like(den))
    return torch.ones(w.shape[0], dtype=w.dtype, device=w.device)


def lookup_sparse(ids, weights, weight, combiner="sum"):
    """(out [B, nOutput], scales [B]): out[b] = s_b * sum_k w_k * weight[id_k - 1] over row b's in-range ids
    (1-based, the values of the sparse ``ids``); ``weights`` shares the pattern of ``ids`` or is None (w = 1).
    s_b = 1 (sum), 1 / sum w (mean), 1 / sqrt(sum w^2) (sqrtn), 0 for a row without ids. ``ids`` may also be a
    dense [B, L] tensor (0 = no id), which takes the torch form."""
    if combiner not in COMBINERS:
        raise ValueError(f"combiner must be one of {sorted(COMBINERS)}, got {combiner!r}")
    sparse_in = _is_coo(ids) or isinstance(ids, Coo)
    if sparse_in:
        ids = coo(ids)
        weights = None if weights is None else coo(weights)
    if (sparse_in and native_on(ids.idx.is_cuda) and _f32_gpu(weight)
            and (weights is None or (weights.nnz == ids.nnz and weights.shape == ids.shape))):
        _set_route("lookup_sparse", "native")
        B, nOut = ids.shape[0], weight.shape[1]
        if ids.nnz == 0:
            out = torch.zeros(B, nOut, dtype=torch.float32, device=weight.device)
            return out, torch.full((B,), 1.0 if combiner == "sum" else 0.0, dtype=torch.float32, device=weight.device)
        out = torch.empty(B, nOut, dtype=torch.float32, device=weight.device)
        scales = torch.empty(B, dtype=torch.float32, device=weight.device)
        native.get().lookup_sparse_fwd(ids.offs, ids.vals, None if weights is None else weights.vals,
                                       weight.contiguous(), COMBINERS[combiner], out, scales)
        return out, scales
    _set_route("lookup_sparse", "torch")
    idx, w = _dense_ids(ids, weights, weight.shape[0], weight.dtype)
    scales = _row_scale(w, combiner)
    out = (weight[idx] * w.unsqueeze(-1)).sum(1) * scales.unsqueeze(1)
    return out, scales


def lookup_sparse_backward(ids, weights, scales, gy, gradWeight, scale=1.0):
    """gradWeight[id_k - 1] += scale * s_b * w_k * gy[b], in place (``scales`` = the forward's s_b)."""
    sparse_in = _is_coo(ids) or isinstance(ids, Coo)
    if sparse_in:
        ids = coo(ids)
        weights = None if weights is None else coo(weights)
    if (sparse_in and native_on(ids.idx.is_cuda) and _f32_gpu(gy, gradWeight, scales) and gradWeight.is_contiguous()
            and (weights is None or (weights.nnz == ids.nnz and weights.shape == ids.shape))):
        if ids.nnz == 0 or scale == 0:
            _set_route("lookup_sparse_backward", "ordered" if native.deterministic() else "native")
            return gradWeight
        r = native.get().lookup_sparse_bwd(ids.idx, ids.offs, ids.vals, None if weights is None else weights.vals,
                                           scales.contiguous(), gy.contiguous(), gradWeight, float(scale))
        _set_route("lookup_sparse_backward", "ordered" if r else "native")
        return gradWeight
    _set_route("lookup_sparse_backward", "torch")
    idx, w = _dense_ids(ids, weights, gradWeight.shape[0], gradWeight.dtype)
    coef = w * scales.to(w.dtype).unsqueeze(1)                                       # [B, L]
    src = (coef.unsqueeze(-1) * gy.to(w.dtype).unsqueeze(1)).reshape(-1, gy.shape[1])    # [B L, nOutput]
    gradWeight.index_add_(0, idx.reshape(-1), src, alpha=scale)
    return gradWeight


# ------------------------------------------------------------------------------------------------- SparseJoinTable
def concat_cols(tensors):
    """Join of 2-D sparse tensors [B, D_i] along the columns: a coalesced sparse [B, sum D_i]."""
    tensors = [t.x if isinstance(t, Coo) else t for t in tensors]
    if (0 < len(tensors) <= MAX_JOIN and all(_is_coo(t) and t.shape[0] == tensors[0].shape[0] for t in tensors)
            and native_on(all(t.is_cuda for t in tensors))):
        _set_route("concat_cols", "native")
        cs = [Coo(t) for t in tensors]
        B, total, dev = cs[0].shape[0], sum(c.nnz for c in cs), cs[0].idx.device
        # zero-filled: the slots that entries with a row outside [0, B) would have taken are never written
        idx = torch.zeros(2, total, dtype=torch.int64, device=dev)
        vals = torch.zeros(total, dtype=torch.float32, device=dev)
        if total:
            native.get().sparse_concat_cols([c.idx for c in cs], [c.vals for c in cs], [c.offs for c in cs],
                                            [c.shape[1] for c in cs], idx, vals)
        return torch.sparse_coo_tensor(idx, vals, (B, sum(c.shape[1] for c in cs)), is_coalesced=True)
    _set_route("concat_cols", "torch")
    return torch.cat([t.to_dense() for t in tensors], dim=1).to_sparse()
