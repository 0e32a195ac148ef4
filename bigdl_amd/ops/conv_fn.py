"""Differentiable convolutions on the native implicit-GEMM kernels (csrc/conv_igemm.hip) for the long tail of
conv-shaped layers that are written as autograd functions (``AutogradModule.fn``): transposed ("full")
convolution, temporal (1-D) convolution, connection-table convolution, the pointwise half of separable
convolution and volumetric (3-D) convolution — so none of them falls back to a vendor library on the GPU.

Every function takes / returns fp32 NCHW tensors like the layers' reference math; inside, activations run as
bf16 NHWC with channels zero-padded to multiples of 8 (the kernels' 16-byte granule) and fp32 accumulation.

    conv2d(x, w, b, stride, pad, dil)           y = x (*) w        fwd: NT GEMM, bwd: dgrad + wgrad kernels
    conv_transpose2d(x, w, b, stride, pad, adj) y = x (*)^T w      fwd: the dgrad kernel, bwd: fwd + wgrad
    conv3d(x, w, b, stride, pad)                native 3-D implicit GEMM (csrc/conv3d.hip), one launch per direction
    conv_transpose3d(x, w, b, stride, pad, adj) fwd: the 3-D dgrad kernel, bwd: 3-D fwd + wgrad
    separable_conv2d(x, wd, wp, b, stride, pad) depthwise + pointwise; fused forward (csrc/sepconv.hip) when switched on

The 3-D functions run bf16 NDHWC operands with fp32 results (every tap accumulated in fp32, nothing rounded to bf16
afterwards); the weight gradient's voxel splits are summed in fixed order, so it is deterministic.
BIGDL_CONV3D_NATIVE=0 (read at import) selects the older path instead: one 2-D convolution per temporal tap on
depth-gathered batches, which also serves geometries the 3-D kernels do not take (pad >= kernel extent).

Reference: S/nn/SpatialConvolution.scala, SpatialFullConvolution.scala:71, TemporalConvolution.scala,
SpatialConvolutionMap.scala, SpatialSeparableConvolution.scala:54, VolumetricConvolution.scala:51.
"""
import math
import os

import torch
import torch.nn.functional as F

from . import conv as cv


def _zeros(*shape, **kw):
    from . import zeros

    return zeros(*shape, **kw)

BF16 = torch.bfloat16
CL = torch.channels_last


def _p8(n):
    return -(-n // 8) * 8


def _act16(x, C8):
    """fp32/bf16 NCHW -> bf16 NHWC with C padded to C8."""
    y = x.to(BF16).contiguous(memory_format=CL)
    if C8 != x.shape[1]:
        y = F.pad(y, (0, 0, 0, 0, 0, C8 - x.shape[1])).contiguous(memory_format=CL)
    return y


def _w16(w, K8, C8):
    """(K, C, R, S) -> bf16 KRSC (channels_last) padded to (K8, C8, R, S)."""
    K, C = w.shape[0], w.shape[1]
    w = w.to(BF16)
    if K8 != K or C8 != C:
        w = F.pad(w, (0, 0, 0, 0, 0, C8 - C, 0, K8 - K))
    return w.contiguous(memory_format=CL)


def _out_size(H, k, s, p, d):
    return (H + 2 * p - d * (k - 1) - 1) // s + 1


class _Conv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, stride, pad, dil):
        K, C = w.shape[0], w.shape[1]
        C8, K8 = _p8(C), _p8(K)
        x16 = _act16(x, C8)
        w16 = _w16(w, K8, C8)
        bias = None
        if b is not None:
            bias = b.float() if K8 == K else F.pad(b.float(), (0, K8 - K))
        y = cv.conv2d_fwd(x16, w16, bias, stride, pad, dil)
        ctx.save_for_backward(x16, w16)
        ctx.geo = (stride, pad, dil, K, C, x.shape, b is not None)
        return y[:, :K].float().contiguous()

    @staticmethod
    def backward(ctx, gy):
        x16, w16 = ctx.saved_tensors
        stride, pad, dil, K, C, xshape, has_b = ctx.geo
        K8, C8 = w16.shape[0], w16.shape[1]
        gy16 = _act16(gy, K8)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gi = cv.conv2d_dgrad(gy16, cv.transpose_w(w16), (xshape[0], C8, xshape[2], xshape[3]), stride, pad, dil)
            gx = gi[:, :C].float().contiguous()
        if ctx.needs_input_grad[1] or (has_b and ctx.needs_input_grad[2]):
            dw = _zeros(w16.shape, device=gy.device, memory_format=CL)
            db = _zeros(K8, device=gy.device) if has_b else None
            cv.conv2d_wgrad(gy16, x16, dw, db, stride, pad, dil)
            gw = dw[:K, :C].contiguous()
            gb = db[:K] if has_b else None
        return gx, gw, gb, None, None, None


def conv2d(x, w, b=None, stride=(1, 1), pad=(0, 0), dil=(1, 1)):
    """Native 2-D convolution (fp32 NCHW in / out). Falls back to torch on the CPU engine."""
    if not x.is_cuda:
        return F.conv2d(x, w, b, stride, pad, dil)
    return _Conv2d.apply(x, w, b, tuple(stride), tuple(pad), tuple(dil))


class _ConvT2d(torch.autograd.Function):
    """y = conv_transpose(x, w): exactly the data gradient of the conv that maps y's shape to x's with weight w
    (w: [Cin, Cout, kh, kw] is that conv's [K, C, R, S])."""

    @staticmethod
    def forward(ctx, x, w, b, stride, pad, adj):
        Cin, Cout, kh, kw = w.shape
        N, _, H, W = x.shape
        OH = (H - 1) * stride[0] - 2 * pad[0] + kh + adj[0]
        OW = (W - 1) * stride[1] - 2 * pad[1] + kw + adj[1]
        K8, C8 = _p8(Cin), _p8(Cout)
        x16 = _act16(x, K8)
        w16 = _w16(w, K8, C8)
        y16 = cv.conv2d_dgrad(x16, cv.transpose_w(w16), (N, C8, OH, OW), stride, pad)
        y = y16[:, :Cout].float()
        if b is not None:
            y = y + b.view(1, -1, 1, 1)
        ctx.save_for_backward(x16, w16)
        ctx.geo = (stride, pad, Cin, Cout, b is not None)
        return y.contiguous()

    @staticmethod
    def backward(ctx, gy):
        x16, w16 = ctx.saved_tensors
        stride, pad, Cin, Cout, has_b = ctx.geo
        K8, C8 = w16.shape[0], w16.shape[1]
        gy16 = _act16(gy, C8)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            # the forward of the underlying conv (input = gy, output grid = x's)
            gi = cv.conv2d_fwd(gy16, w16, None, stride, pad)
            gx = gi[:, :Cin, :x16.shape[2], :x16.shape[3]].float().contiguous()
        if ctx.needs_input_grad[1]:
            dw = _zeros(w16.shape, device=gy.device, memory_format=CL)
            cv.conv2d_wgrad(x16, gy16, dw, None, stride, pad)
            gw = dw[:Cin, :Cout].contiguous()
        if has_b and ctx.needs_input_grad[2]:
            gb = gy.sum(dim=(0, 2, 3))
        return gx, gw, gb, None, None, None


def conv_transpose2d(x, w, b=None, stride=(1, 1), pad=(0, 0), adj=(0, 0)):
    if not x.is_cuda:
        return F.conv_transpose2d(x, w, b, stride, pad, adj)
    return _ConvT2d.apply(x, w, b, tuple(stride), tuple(pad), tuple(adj))


def linear(x, w, b=None):
    """y = x W^T + b over the last dimension on the MFMA GEMM kernels (a 1x1 convolution over the rows): the
    projections of layers written as autograd functions (attention, generic recurrent cells). CPU: torch."""
    if not x.is_cuda:
        return F.linear(x, w, b)
    lead = x.shape[:-1]
    rows = x.reshape(-1, x.shape[-1])
    y = conv2d(rows.view(rows.shape[0], rows.shape[1], 1, 1), w.view(w.shape[0], w.shape[1], 1, 1), b)
    return y.view(*lead, w.shape[0])


class _GroupConv(torch.autograd.Function):
    """Grouped / depthwise convolution in one launch per pass (csrc/grouped_conv.hip), fp32 NCHW."""

    @staticmethod
    def forward(ctx, x, w, b, stride, pad, dil, groups):
        from . import native

        x, w = x.float().contiguous(), w.float().contiguous()
        N, C, H, W = x.shape
        K, _, R, S = w.shape
        OH = (H + 2 * pad[0] - dil[0] * (R - 1) - 1) // stride[0] + 1
        OW = (W + 2 * pad[1] - dil[1] * (S - 1) - 1) // stride[1] + 1
        y = x.new_empty(N, K, OH, OW)
        geo = [stride[0], stride[1], pad[0], pad[1], dil[0], dil[1], groups]
        native.get().gconv(0, x, w, b.float().contiguous() if b is not None else None, y, geo)
        ctx.save_for_backward(x, w)
        ctx.geo, ctx.has_b = geo, b is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        from . import native

        x, w = ctx.saved_tensors
        gy = gy.float().contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            native.get().gconv(1, gx, w, None, gy, ctx.geo)
        if ctx.needs_input_grad[1] or (ctx.has_b and ctx.needs_input_grad[2]):
            gw = torch.zeros_like(w)
            gb = torch.zeros(w.shape[0], device=x.device) if ctx.has_b else None
            native.get().gconv(2, x, gw, gb, gy, ctx.geo)
        return gx, gw, gb, None, None, None, None


# Grouped convolution on MFMA, every group in one launch per direction (csrc/gconv_mfma.hip), is opt-in:
# BIGDL_GCONV_MFMA=1, set_gconv_mfma, or the Engine property bigdl.gconv.mfma. Unset means DEFAULT_GCONV_MFMA (the
# direct kernel up to 16 input channels per group, else one implicit-GEMM convolution per group).
DEFAULT_GCONV_MFMA = False
_GCONV_MFMA = [None]
_GROUP_ROUTE = [None]


def set_gconv_mfma(v):
    """True / False, "1" / "0", or None for the default."""
    _GCONV_MFMA[0] = None if v is None or v == "" else str(v).lower() in ("1", "true", "yes")


def gconv_mfma():
    v = _GCONV_MFMA[0]
    if v is None:
        env = os.environ.get("BIGDL_GCONV_MFMA", "")
        v = DEFAULT_GCONV_MFMA if env == "" else env.lower() in ("1", "true", "yes")
    return bool(v)


def last_group_route():
    """"mfma", "direct" or "loop": what the last grouped convolution on the GPU ran (None before the first)."""
    return _GROUP_ROUTE[0]


def group_geo(stride, pad, dil, groups):
    return [stride[0], stride[1], pad[0], pad[1], dil[0], dil[1], groups]


def group_route(xshape, wshape, stride, pad, dil, groups):
    """The route of a grouped convolution of an input of ``xshape`` with a (K, C / groups, R, S) weight; recorded for
    last_group_route(). "mfma" when the route is switched on and the kernels take the geometry."""
    route = "direct" if xshape[1] // groups <= 16 else "loop"
    if gconv_mfma():
        from . import native

        if native.get().gconv_mfma_supported(xshape[0], xshape[1], xshape[2], xshape[3], wshape[0], wshape[2],
                                             wshape[3], group_geo(stride, pad, dil, groups)):
            route = "mfma"
    _GROUP_ROUTE[0] = route
    return route


def group_transpose_w(w16, groups):
    """(K, C / G, R, S) channels_last bf16 -> contiguous (C, R, S, K / G): each group's weight transposed for the
    grouped data-gradient kernel."""
    K, cin_g, R, S = w16.shape
    w = w16.permute(0, 2, 3, 1).reshape(groups, K // groups, R, S, cin_g)
    return w.permute(0, 4, 2, 3, 1).reshape(groups * cin_g, R, S, K // groups).contiguous()


def group_wgrad(gy16, x16, wshape, geo, want_db):
    """fp32 dw (channels_last, shaped like the weight) and db of a grouped convolution: one launch plus the
    fixed-order sum of its pixel splits."""
    from . import native

    C = native.get()
    dw = _zeros(*wshape, device=gy16.device, memory_format=CL)
    db = _zeros(wshape[0], device=gy16.device) if want_db else None
    splits = C.gconv_mfma_wgrad_splits(gy16, x16, dw, geo)
    ws = torch.empty(splits * (dw.numel() + wshape[0]), dtype=torch.float32, device=gy16.device)
    C.gconv_mfma_wgrad(gy16, x16, dw, db, ws, geo)
    return dw, db


class _GroupConvMfma(torch.autograd.Function):
    """Grouped convolution on csrc/gconv_mfma.hip: bf16 NHWC operands over all channels, fp32 results, one launch per
    direction for every group."""

    @staticmethod
    def forward(ctx, x, w, b, stride, pad, dil, groups):
        from . import native

        N, C, H, W = x.shape
        K, cin_g, R, S = w.shape
        OH, OW = _out_size(H, R, stride[0], pad[0], dil[0]), _out_size(W, S, stride[1], pad[1], dil[1])
        x16, w16 = _act16(x, C), _w16(w, K, cin_g)
        geo = group_geo(stride, pad, dil, groups)
        y = torch.empty((N, K, OH, OW), dtype=torch.float32, device=x.device, memory_format=CL)
        native.get().gconv_mfma_fwd(x16, w16, b.float().contiguous() if b is not None else None, y, False, geo)
        ctx.save_for_backward(x16, w16)
        ctx.geo, ctx.has_b = geo, b is not None
        return y.contiguous()

    @staticmethod
    def backward(ctx, gy):
        from . import native

        x16, w16 = ctx.saved_tensors
        geo = ctx.geo
        gy16 = _act16(gy, gy.shape[1])
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gi = torch.empty(x16.shape, dtype=torch.float32, device=gy.device, memory_format=CL)
            native.get().gconv_mfma_dgrad(gy16, group_transpose_w(w16, geo[6]), gi, geo)
            gx = gi.contiguous()
        if ctx.needs_input_grad[1] or (ctx.has_b and ctx.needs_input_grad[2]):
            dw, gb = group_wgrad(gy16, x16, w16.shape, geo, ctx.has_b)
            gw = dw.contiguous()
        return gx, gw, gb, None, None, None, None


def group_conv2d(x, w, b=None, stride=(1, 1), pad=(0, 0), dil=(1, 1), groups=1):
    """Grouped convolution. With the MFMA route switched on and a geometry it takes (last_group_route() == "mfma"):
    every group in one launch per direction. Else the direct kernel when groups carry little reduction depth
    (depthwise, <= 16 input channels per group: "direct"), else the implicit-GEMM conv per group writing its channel
    slice ("loop")."""
    if not x.is_cuda:
        return F.conv2d(x, w, b, stride, pad, dil, groups)
    if groups == 1:
        return conv2d(x, w, b, stride, pad, dil)
    route = group_route(x.shape, w.shape, stride, pad, dil, groups)
    if route == "mfma":
        return _GroupConvMfma.apply(x, w, b, tuple(stride), tuple(pad), tuple(dil), groups)
    cin_g = x.shape[1] // groups
    if route == "direct":
        return _GroupConv.apply(x, w, b, tuple(stride), tuple(pad), tuple(dil), groups)
    cout_g = w.shape[0] // groups
    outs = [conv2d(x[:, g * cin_g:(g + 1) * cin_g], w[g * cout_g:(g + 1) * cout_g],
                   b[g * cout_g:(g + 1) * cout_g] if b is not None else None, stride, pad, dil) for g in range(groups)]
    return torch.cat(outs, 1)


# The fused depthwise-separable forward (csrc/sepconv.hip) is opt-in: BIGDL_SEPCONV_FUSED=1, set_sepconv_fused, or the
# Engine property bigdl.sepconv.fused. Unset means DEFAULT_SEPCONV_FUSED (the depthwise kernel + the pointwise GEMM).
DEFAULT_SEPCONV_FUSED = False
_SEPCONV_FUSED = [None]
_SEPARABLE_ROUTE = [None]


def set_sepconv_fused(v):
    """True / False, "1" / "0", or None for the default."""
    _SEPCONV_FUSED[0] = None if v is None or v == "" else str(v).lower() in ("1", "true", "yes")


def sepconv_fused():
    v = _SEPCONV_FUSED[0]
    if v is None:
        env = os.environ.get("BIGDL_SEPCONV_FUSED", "")
        v = DEFAULT_SEPCONV_FUSED if env == "" else env.lower() in ("1", "true", "yes")
    return bool(v)


def last_separable_route():
    """"fused" or "split": what the last separable_conv2d call on the GPU ran (None before the first)."""
    return _SEPARABLE_ROUTE[0]


class _SepConv(torch.autograd.Function):
    """Depthwise + pointwise convolution, forward in ONE launch (csrc/sepconv.hip): the depthwise result lives in LDS
    and feeds the pointwise MFMA GEMM. Training keeps its bf16 NHWC rounding (mid16, written by the same launch) for the
    pointwise weight gradient; the backward runs the kernels of the two-kernel path on it."""

    @staticmethod
    def forward(ctx, x, wd, wp, b, stride, pad):
        from . import native

        x, wd = x.float().contiguous(), wd.float().contiguous()
        N, Cin, H, W = x.shape
        Cmid, K = wd.shape[0], wp.shape[0]
        C8, K8, C32 = _p8(Cmid), _p8(K), -(-Cmid // 32) * 32
        OH = _out_size(H, wd.shape[2], stride[0], pad[0], 1)
        OW = _out_size(W, wd.shape[3], stride[1], pad[1], 1)
        wp32 = _zeros(K8, C32, dtype=BF16, device=x.device)
        wp32[:K, :Cmid].copy_(wp.reshape(K, Cmid))
        y = x.new_empty(N, K, OH, OW)
        train = any(ctx.needs_input_grad[:4])
        mid16 = torch.empty(N, OH, OW, C8, dtype=BF16, device=x.device) if train else None
        native.get().sepconv_fwd(x, wd, wp32, b.float().contiguous() if b is not None else None, y, mid16,
                                 [stride[0], stride[1], pad[0], pad[1]])
        if train:
            ctx.save_for_backward(x, wd, _w16(wp, K8, C8), mid16)
        ctx.geo = (stride, pad, K, Cmid, b is not None)
        return y

    @staticmethod
    def backward(ctx, gy):
        from . import native

        x, wd, w16, mid16 = ctx.saved_tensors
        stride, pad, K, Cmid, has_b = ctx.geo
        K8, C8 = w16.shape[0], w16.shape[1]
        N, OH, OW, _ = mid16.shape
        gy16 = _act16(gy, K8)
        gx = gwd = gwp = gb = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            gm = cv.conv2d_dgrad(gy16, cv.transpose_w(w16), (N, C8, OH, OW), (1, 1), (0, 0))
            gm = gm[:, :Cmid].float().contiguous()
            geo = [stride[0], stride[1], pad[0], pad[1], 1, 1, x.shape[1]]
            if ctx.needs_input_grad[0]:
                gx = torch.empty_like(x)
                native.get().gconv(1, gx, wd, None, gm, geo)
            if ctx.needs_input_grad[1]:
                gwd = torch.zeros_like(wd)
                native.get().gconv(2, x, gwd, None, gm, geo)
        if ctx.needs_input_grad[2] or (has_b and ctx.needs_input_grad[3]):
            dw = _zeros(w16.shape, device=gy.device, memory_format=CL)
            db = _zeros(K8, device=gy.device) if has_b else None
            cv.conv2d_wgrad(gy16, mid16.permute(0, 3, 1, 2), dw, db, (1, 1), (0, 0))
            gwp = dw[:K, :Cmid].contiguous()
            gb = db[:K] if has_b else None
        return gx, gwd, gwp, gb, None, None


def separable_conv2d(x, depth_w, point_w, bias=None, stride=(1, 1), pad=(0, 0)):
    """y = conv1x1(depthwise(x, depth_w), point_w) + bias; depth_w [Cin * dm, 1, kH, kW], point_w [Cout, Cin * dm, 1,
    1]. GPU: the fused forward when it is switched on and takes the geometry (last_separable_route() == "fused"), else
    the depthwise kernel followed by the pointwise GEMM ("split"). CPU engine: torch."""
    cin = x.shape[1]
    if not x.is_cuda:
        return F.conv2d(F.conv2d(x, depth_w, None, stride, pad, 1, cin), point_w, bias)
    if sepconv_fused() and depth_w.shape[1] == 1 and depth_w.shape[0] % cin == 0:
        from . import native

        N, _, H, W = x.shape
        if native.get().sepconv_supported(N, cin, H, W, depth_w.shape[0] // cin, point_w.shape[0], depth_w.shape[2],
                                          depth_w.shape[3], [stride[0], stride[1], pad[0], pad[1]]):
            _SEPARABLE_ROUTE[0] = "fused"
            return _SepConv.apply(x, depth_w, point_w, bias, tuple(stride), tuple(pad))
    _SEPARABLE_ROUTE[0] = "split"
    return conv2d(group_conv2d(x, depth_w, None, stride, pad, groups=cin), point_w, bias)


def conv1d(x, w, b=None, stride=1):
    """x: [N, C, L], w: [K, C, kW] -> [N, K, L'] as a 2-D convolution over a height-1 image."""
    if not x.is_cuda:
        return F.conv1d(x, w, b, stride)
    return conv2d(x.unsqueeze(2), w.unsqueeze(2), b, (1, stride), (0, 0)).squeeze(2)


def _ndhwc16(x, C8):
    """fp32/bf16 NCDHW -> contiguous bf16 [N][T][H][W][C8] (channels zero-padded) in one copy."""
    N, C, T, H, W = x.shape
    y = torch.empty(N, T, H, W, C8, dtype=BF16, device=x.device)
    y[..., :C].copy_(x.permute(0, 2, 3, 4, 1))
    if C8 != C:
        y[..., C:].zero_()
    return y


def _w3d16(w, K8, C8):
    """(K, C, kT, kH, kW) -> contiguous bf16 [K8][kT][kH][kW][C8], zero-padded."""
    K, C = w.shape[0], w.shape[1]
    y = _zeros(K8, *w.shape[2:], C8, dtype=BF16, device=w.device)
    y[:K, ..., :C].copy_(w.permute(0, 2, 3, 4, 1))
    return y


def _ncdhw(y, C):
    """fp32 [N][T][H][W][C8] -> contiguous NCDHW over the first C channels."""
    return y[..., :C].permute(0, 4, 1, 2, 3).contiguous()


def _pad_bias(b, K, K8):
    if b is None:
        return None
    return b.float().contiguous() if K8 == K else F.pad(b.float(), (0, K8 - K))


def _wgrad3d(dy16, x16, wshape, geo, want_db):
    """dw [K8][kT][kH][kW][C8] (and db [K8]) of the convolution x16 -> dy16's grid: one launch plus the fixed-order
    sum of its voxel splits."""
    from . import native

    C = native.get()
    dw = _zeros(wshape, device=dy16.device)
    db = _zeros(wshape[0], device=dy16.device) if want_db else None
    splits = C.conv3d_wgrad_splits(dy16, x16, dw, geo)
    ws = torch.empty(splits * (dw.numel() + wshape[0]), dtype=torch.float32, device=dy16.device)
    C.conv3d_wgrad(dy16, x16, dw, db, ws, geo)
    return dw, db


class _Conv3d(torch.autograd.Function):
    """Volumetric convolution on csrc/conv3d.hip: one launch per direction, fp32 results."""

    @staticmethod
    def forward(ctx, x, w, b, stride, pad):
        from . import native

        K, C = w.shape[0], w.shape[1]
        K8, C8 = _p8(K), _p8(C)
        N, _, T, H, W = x.shape
        OT, OH, OW = (_out_size(e, k, s, p, 1) for e, k, s, p in zip((T, H, W), w.shape[2:], stride, pad))
        x16, w16 = _ndhwc16(x, C8), _w3d16(w, K8, C8)
        geo = list(stride) + list(pad)
        y = torch.empty(N, OT, OH, OW, K8, dtype=torch.float32, device=x.device)
        native.get().conv3d_fwd(x16, w16, _pad_bias(b, K, K8), y, geo)
        ctx.save_for_backward(x16, w16)
        ctx.geo = (geo, K, C, b is not None)
        return _ncdhw(y, K)

    @staticmethod
    def backward(ctx, gy):
        from . import native

        x16, w16 = ctx.saved_tensors
        geo, K, C, has_b = ctx.geo
        gy16 = _ndhwc16(gy, w16.shape[0])
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gi = torch.empty(x16.shape, dtype=torch.float32, device=gy.device)
            native.get().conv3d_dgrad(gy16, w16.permute(4, 1, 2, 3, 0).contiguous(), None, gi, geo)
            gx = _ncdhw(gi, C)
        if ctx.needs_input_grad[1] or (has_b and ctx.needs_input_grad[2]):
            dw, db = _wgrad3d(gy16, x16, w16.shape, geo, has_b)
            gw = dw[:K, ..., :C].permute(0, 4, 1, 2, 3).contiguous()
            gb = db[:K] if has_b else None
        return gx, gw, gb, None, None


class _ConvT3d(torch.autograd.Function):
    """y = conv_transpose3d(x, w): the data gradient of the convolution that maps y's grid to x's with weight w
    (w: [Cin, Cout, kT, kH, kW] is that convolution's [K, C, kT, kH, kW]); the bias is added in the kernel."""

    @staticmethod
    def forward(ctx, x, w, b, stride, pad, adj):
        from . import native

        Cin, Cout = w.shape[0], w.shape[1]
        K8, C8 = _p8(Cin), _p8(Cout)
        N = x.shape[0]
        OT, OH, OW = ((e - 1) * s - 2 * p + k + a for e, k, s, p, a in zip(x.shape[2:], w.shape[2:], stride, pad, adj))
        x16, w16 = _ndhwc16(x, K8), _w3d16(w, K8, C8)
        geo = list(stride) + list(pad)
        y = torch.empty(N, OT, OH, OW, C8, dtype=torch.float32, device=x.device)
        native.get().conv3d_dgrad(x16, w16.permute(4, 1, 2, 3, 0).contiguous(), _pad_bias(b, Cout, C8), y, geo)
        ctx.save_for_backward(x16, w16)
        ctx.geo = (geo, Cin, Cout, b is not None)
        return _ncdhw(y, Cout)

    @staticmethod
    def backward(ctx, gy):
        from . import native

        x16, w16 = ctx.saved_tensors
        geo, Cin, Cout, has_b = ctx.geo
        gy16 = _ndhwc16(gy, w16.shape[4])
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            # the forward of the underlying convolution (input = gy, output grid = x's)
            gi = torch.empty(x16.shape, dtype=torch.float32, device=gy.device)
            native.get().conv3d_fwd(gy16, w16, None, gi, geo)
            gx = _ncdhw(gi, Cin)
        if ctx.needs_input_grad[1]:
            dw, _ = _wgrad3d(x16, gy16, w16.shape, geo, False)
            gw = dw[:Cin, ..., :Cout].permute(0, 4, 1, 2, 3).contiguous()
        if has_b and ctx.needs_input_grad[2]:
            gb = gy.sum(dim=(0, 2, 3, 4))
        return gx, gw, gb, None, None, None


# BIGDL_CONV3D_NATIVE=0 keeps 3-D convolution on the per-temporal-tap 2-D path below
CONV3D_NATIVE = [os.environ.get("BIGDL_CONV3D_NATIVE", "1") != "0"]


def _native3d(x, w, stride, pad, adj=None):
    """What csrc/conv3d.hip takes (its geo_ok): strides >= 1, 0 <= pad < kernel extent, adj < stride, no empty
    extent on either grid, and fewer than 2^31 elements in each padded operand. adj is given for the transposed
    convolution, whose x lives on the underlying convolution's output grid."""
    k = w.shape[2:]
    if not (CONV3D_NATIVE[0] and all(s >= 1 for s in stride) and all(0 <= p < e for p, e in zip(pad, k))):
        return False
    if adj is None:
        other = [_out_size(e, kk, s, p, 1) for e, kk, s, p in zip(x.shape[2:], k, stride, pad)]
    elif all(0 <= a < s for a, s in zip(adj, stride)):
        other = [(e - 1) * s - 2 * p + kk + a for e, kk, s, p, a in zip(x.shape[2:], k, stride, pad, adj)]
    else:
        return False
    if min(x.shape) < 1 or min(w.shape) < 1 or min(other) < 1 or math.prod(stride) > 65535:   # phases ride grid.z
        return False
    c_x, c_other = (_p8(w.shape[1]), _p8(w.shape[0])) if adj is None else (_p8(w.shape[0]), _p8(w.shape[1]))
    vox_x, vox_other, lim = x.shape[0] * math.prod(x.shape[2:]), x.shape[0] * math.prod(other), 1 << 31
    return vox_x * c_x < lim and vox_other * c_other < lim and math.prod(k) * c_x * c_other < lim


def conv_transpose3d(x, w, b=None, stride=(1, 1, 1), pad=(0, 0, 0), adj=(0, 0, 0)):
    """x: [N, Cin, T, H, W], w: [Cin, Cout, kT, kH, kW]: the native data-gradient kernel run forward."""
    if not x.is_cuda:
        return F.conv_transpose3d(x, w, b, stride, pad, adj)
    if _native3d(x, w, stride, pad, tuple(adj)):
        return _ConvT3d.apply(x, w, b, tuple(stride), tuple(pad), tuple(adj))
    return _conv_transpose3d_taps(x, w, b, stride, pad, adj)


def conv3d(x, w, b=None, stride=(1, 1, 1), pad=(0, 0, 0)):
    """x: [N, C, T, H, W], w: [K, C, kT, kH, kW]: one native launch per direction."""
    if not x.is_cuda:
        return F.conv3d(x, w, b, stride, pad)
    if _native3d(x, w, stride, pad):
        return _Conv3d.apply(x, w, b, tuple(stride), tuple(pad))
    return _conv3d_taps(x, w, b, stride, pad)


def _conv_transpose3d_taps(x, w, b, stride, pad, adj):
    """Per-tap alternative: input frame t feeds output frames t*sT + kt - pT, so each temporal tap kt is a native 2-D
    transposed convolution of all frames (folded into the batch), scattered into the output frames with index_add
    (the adjoint of _conv3d_taps' depth gather)."""
    N, Cin, T, H, W = x.shape
    _, Cout, kT, kH, kW = w.shape
    sT, sH, sW = stride
    pT, pH, pW = pad
    OT = (T - 1) * sT - 2 * pT + kT + adj[0]
    L = max((T - 1) * sT + kT, pT + OT)                 # padded temporal extent
    xs = x.permute(0, 2, 1, 3, 4).reshape(N * T, Cin, H, W)
    y = None
    for kt in range(kT):
        part = conv_transpose2d(xs, w[:, :, kt], None, (sH, sW), (pH, pW), (adj[1], adj[2]))
        OH, OW = part.shape[2], part.shape[3]
        if y is None:
            y = part.new_zeros(N, L, Cout, OH, OW)
        idx = torch.arange(T, device=x.device) * sT + kt
        y = y.index_add(1, idx, part.view(N, T, Cout, OH, OW))
    y = y[:, pT:pT + OT].permute(0, 2, 1, 3, 4)
    if b is not None:
        y = y + b.view(1, -1, 1, 1, 1)
    return y.contiguous()


def _conv3d_taps(x, w, b, stride, pad):
    """Per-tap alternative: each temporal tap kt is a 2-D convolution of the depth slices t*sT + kt - pT (zero
    outside) folded into the batch; the kT partial outputs are summed."""
    N, C, T, H, W = x.shape
    K, _, kT, kH, kW = w.shape
    sT, sH, sW = stride
    pT, pH, pW = pad
    OT = (T + 2 * pT - kT) // sT + 1
    xp = F.pad(x, (0, 0, 0, 0, pT, pT)) if pT else x
    y = None
    for kt in range(kT):
        idx = torch.arange(OT, device=x.device) * sT + kt
        xs = xp.index_select(2, idx).permute(0, 2, 1, 3, 4).reshape(N * OT, C, H, W)
        part = conv2d(xs, w[:, :, kt], b if kt == 0 else None, (sH, sW), (pH, pW))
        y = part if y is None else y + part
    OH, OW = y.shape[2], y.shape[3]
    return y.view(N, OT, K, OH, OW).permute(0, 2, 1, 3, 4).contiguous()
