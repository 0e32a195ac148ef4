"""Detection primitives: NMS, RoiAlign, RoiPooling (device dispatch) and the bounding-box utilities.

Reference: S/nn/Nms.scala:26-236, S/nn/RoiAlign.scala:45-420, S/nn/RoiPooling.scala:42-366,
S/transform/vision/image/util/BboxUtil.scala:26-581.

On a GPU tensor the HIP kernels in csrc/detection.hip run (IoU bitmask NMS with a single-wave greedy scan,
one-thread-per-output RoiAlign / RoiPooling; ``multiclass_nms`` and ``roi_align_levels`` cover all classes of all
images, or all pyramid levels, in one launch each); on the CPU the same arithmetic runs in numpy / torch. Box
conventions follow the reference: pixel boxes use ``+1`` widths (``(x2 - x1 + 1)``) unless ``normalized``.
"""
import collections
import math
import os

import numpy as np
import torch

from . import native


def _on_gpu(t):
    return t.is_cuda


# ------------------------------------------------------------------------------------------------ NMS
def nms_sorted(boxes, thresh, normalized=False, max_keep=-1):
    """Greedy NMS over boxes already sorted by descending score. Returns 0-based kept positions (int64)."""
    n = boxes.shape[0]
    if n == 0:
        return torch.zeros(0, dtype=torch.long, device=boxes.device)
    if _on_gpu(boxes):
        b = boxes.float().contiguous()
        keep = torch.empty(n, dtype=torch.int32, device=b.device)
        cnt = torch.empty(1, dtype=torch.int32, device=b.device)
        native.get().nms(b, float(thresh), bool(normalized), int(max_keep), keep, cnt)
        return keep[: int(cnt.item())].long()
    b = boxes.detach().double().cpu().numpy()
    one = 0.0 if normalized else 1.0
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    areas = (x2 - x1 + one) * (y2 - y1 + one)
    w = np.minimum(x2[:, None], x2[None, :]) - np.maximum(x1[:, None], x1[None, :]) + one
    h = np.minimum(y2[:, None], y2[None, :]) - np.maximum(y1[:, None], y1[None, :]) + one
    inter = w * h
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter / (areas[:, None] + areas[None, :] - inter)
    sup = (w >= 0) & (h >= 0) & (iou > thresh)
    removed = np.zeros(n, dtype=bool)
    keep = []
    for i in range(n):
        if removed[i]:
            continue
        keep.append(i)
        if 0 < max_keep <= len(keep):
            break
        removed |= sup[i]
    return torch.as_tensor(keep, dtype=torch.long, device=boxes.device)


def nms(scores, boxes, thresh, sorted=False, orderWithBBox=False, normalized=False, max_keep=-1):
    """Reference ``Nms.nms``: returns 0-based indices of kept boxes (score order, or box order with
    ``orderWithBBox``)."""
    scores = scores.reshape(-1)
    if scores.numel() == 0:
        return torch.zeros(0, dtype=torch.long, device=scores.device)
    order = torch.arange(scores.numel(), device=scores.device) if sorted else \
        torch.sort(scores, descending=True, stable=True).indices
    kept = order[nms_sorted(boxes[order], thresh, normalized, max_keep)]
    if orderWithBBox:
        kept = torch.sort(kept).values
    return kept


def nms_fast(scores, boxes, nms_thresh, score_thresh, topk=-1, eta=1.0, normalized=True):
    """Reference ``Nms.nmsFast`` (SSD): score threshold, top-k pre-selection, greedy NMS with an optional
    adaptive threshold (``eta < 1``). Returns 0-based indices in descending-score order."""
    s = scores.reshape(-1)
    cand = torch.nonzero(s >= score_thresh).reshape(-1) if score_thresh > 0 else torch.arange(s.numel(),
                                                                                              device=s.device)
    if cand.numel() == 0:
        return cand
    order = cand[torch.sort(s[cand], descending=True, stable=True).indices]
    if topk > 0:
        order = order[:topk]
    if eta >= 1.0:
        return order[nms_sorted(boxes[order], nms_thresh, normalized)]
    b = boxes[order].double().cpu().numpy()
    one = 0.0 if normalized else 1.0
    areas = (b[:, 2] - b[:, 0] + one) * (b[:, 3] - b[:, 1] + one)
    keep, thr = [], nms_thresh
    for i in range(b.shape[0]):
        ok = True
        for k in keep:
            w = min(b[i, 2], b[k, 2]) - max(b[i, 0], b[k, 0]) + one
            h = min(b[i, 3], b[k, 3]) - max(b[i, 1], b[k, 1]) + one
            if w >= 0 and h >= 0:
                inter = w * h
                if inter / (areas[i] + areas[k] - inter) > thr:
                    ok = False
                    break
        if ok:
            keep.append(i)
            if eta < 1 and thr > 0.5:
                thr *= eta
    return order[torch.as_tensor(keep, dtype=torch.long, device=order.device)]


# ------------------------------------------------------------------------------- batched detection ops
# multiclass_nms / roi_align_levels / rpn_select run every (image, class) segment, every pyramid level, or every
# (image, level) segment in one launch per stage (csrc/detection.hip nms_classes_kernel /
# roi_align_levels_fwd_kernel / segmented_topk_*_kernel): BIGDL_DET_BATCHED / Engine property
# bigdl.detection.batched / set_batched; unset means on for GPU tensors (for the RegionProposal module: off, it
# batches only when the switch is set). Off, or on the CPU, the same results come
# from the per-class / per-level loops below, which are also what an overflowing call falls back to.
_BATCHED = [None]
_ROUTE = {"multiclass_nms": None, "roi_align_levels": None, "rpn_select": None, "last": None}
NMS_CLASSES_MIN_CAP = 256                      # smallest LDS capacity nms_classes_kernel is instantiated for


def set_batched(v):
    """True / False, "1" / "0", or None for the engine's default."""
    _BATCHED[0] = None if v is None or v == "" else str(v).lower() in ("1", "true", "yes")


def batched(is_cuda, default=True):
    """Whether a caller with GPU tensors (``is_cuda``) batches; ``default`` is its answer when nothing is set."""
    v = _BATCHED[0]
    if v is None:
        env = os.environ.get("BIGDL_DET_BATCHED", "")
        v = default if env == "" else env.lower() in ("1", "true", "yes")
    return bool(v) and bool(is_cuda)


def last_route(op=None):
    """"batched", "loop" or "overflow": the path the last call of ``op`` ("multiclass_nms" / "roi_align_levels" /
    "rpn_select") took; without ``op``, of whichever of them ran last."""
    return _ROUTE["last" if op is None else op]


def _set_route(op, route):
    _ROUTE[op] = _ROUTE["last"] = route


def _offsets(counts):
    off = [0]
    for n in counts:
        off.append(off[-1] + int(n))
    return off


def _multiclass_nms_loop(scores, boxes, off, score_thresh, nms_thresh, skip_class, inclusive, pre_topk, normalized):
    R, C = scores.shape
    Cb = boxes.shape[1]
    keep = torch.zeros(R, C, dtype=torch.bool, device=scores.device)
    for b in range(len(off) - 1):
        lo, hi = off[b], off[b + 1]
        if hi == lo:
            continue
        for c in range(C):
            if c == skip_class:
                continue
            s, bx = scores[lo:hi, c], boxes[lo:hi, c if Cb > 1 else 0]
            if inclusive:
                kept = nms_fast(s, bx, nms_thresh, score_thresh, pre_topk, 1.0, normalized)
            else:
                cand = torch.nonzero(s > score_thresh).reshape(-1)
                if cand.numel() == 0:
                    continue
                order = cand[torch.sort(s[cand], descending=True, stable=True).indices]
                if pre_topk > 0:
                    order = order[:pre_topk]
                kept = order[nms_sorted(bx[order], nms_thresh, normalized)]
            keep[lo + kept, c] = True
    return keep


def nms_classes_launch(scores, boxes, off, score_thresh, nms_thresh, skip_class, inclusive, pre_topk, normalized,
                       keep, overflow, cap=0):
    """The launch of nms_classes_kernel alone (no read-back, graph-capturable): keep uint8 [R, C] is rewritten in
    full, overflow int32 [1] is set when a segment holds more candidates than the capacity. Returns the capacity."""
    # nms_fast takes every row when its threshold is not positive
    thr = float("-inf") if inclusive and score_thresh <= 0 else float(score_thresh)
    return native.get().nms_classes(scores, boxes, [int(o) for o in off], int(skip_class), thr, bool(inclusive),
                                    int(pre_topk), float(nms_thresh), bool(normalized), keep, overflow, int(cap))


def multiclass_nms(scores, boxes, counts, score_thresh, nms_thresh, skip_class=0, inclusive=False, pre_topk=-1,
                   normalized=False, cap=0):
    """Greedy NMS of every (image, class) segment. scores (R, C); boxes (R, Cb, 4) or (R, Cb * 4) with Cb == C or
    Cb == 1 (class-shared boxes); counts = rows per image. A row is a candidate of its class when
    ``score > score_thresh`` (``>=`` with ``inclusive``, the SSD rule); candidates are taken in descending score
    order (ties: lower row first), cut to ``pre_topk`` when positive, and suppressed greedily at ``nms_thresh``.
    Returns the bool (R, C) mask of kept rows; column ``skip_class`` stays False.

    On the GPU with batching on this is one launch plus the read of the overflow word (the one synchronisation);
    an overflowing call, the CPU, and batching off run the per-class loop, which computes the same mask. ``cap``
    forces the kernel's candidate capacity per segment (256, 1024 or 4096; 0 = from the longest image)."""
    R, C = scores.shape
    boxes = boxes.reshape(R, -1, 4)
    off = _offsets(counts)
    assert off[-1] == R, "multiclass_nms: counts must sum to the number of rows"
    assert boxes.shape[1] in (1, C), "multiclass_nms: boxes must be per class or shared"
    route = "loop"
    if batched(_on_gpu(scores)) and R:
        s, bx = scores.float().contiguous(), boxes.float().contiguous()
        keep = torch.empty(R, C, dtype=torch.uint8, device=s.device)
        overflow = torch.empty(1, dtype=torch.int32, device=s.device)
        nms_classes_launch(s, bx, off, score_thresh, nms_thresh, skip_class, inclusive, pre_topk, normalized, keep,
                           overflow, cap)
        if int(overflow.item()) == 0:
            _set_route("multiclass_nms", "batched")
            return keep.bool()
        route = "overflow"
    keep = _multiclass_nms_loop(scores, boxes, off, score_thresh, nms_thresh, skip_class, inclusive, pre_topk,
                                normalized)
    _set_route("multiclass_nms", route)
    return keep


def _roi_align_levels_loop(fmaps, rois5, levels, scales, sampling_ratio, res):
    C = fmaps[0].shape[1]
    out = torch.zeros(rois5.shape[0], C, res, res, dtype=torch.float32, device=fmaps[0].device)
    lv = levels.clamp(0, len(fmaps) - 1)
    for level in range(len(fmaps)):
        idx = torch.nonzero(lv == level).reshape(-1)
        if idx.numel() == 0:
            continue
        out[idx] = roi_align(fmaps[level], rois5[idx], scales[level], sampling_ratio, res, res)
    return out


def roi_align_levels(fmaps, rois5, levels, scales, sampling_ratio, res):
    """RoiAlign of rois5 (R, 5: batch index, x1, y1, x2, y2) where roi r samples ``fmaps[levels[r]]`` (N, C, H_l,
    W_l) at ``scales[levels[r]]``; levels outside [0, L-1] are clamped. One launch on the GPU with batching on
    (up to 8 levels), the per-level ``roi_align`` loop otherwise; the two are bit-equal. Returns (R, C, res, res)."""
    fmaps = list(fmaps)
    first = fmaps[0]
    R = rois5.shape[0]
    if batched(_on_gpu(first)) and len(fmaps) <= 8:
        out = torch.empty(R, first.shape[1], res, res, dtype=torch.float32, device=first.device)
        if R:
            native.get().roi_align_levels_fwd([f.float().contiguous() for f in fmaps], rois5.float().contiguous(),
                                              levels.to(torch.int32).contiguous(), out,
                                              [float(s) for s in scales], int(sampling_ratio))
        _set_route("roi_align_levels", "batched")
        return out
    _set_route("roi_align_levels", "loop")
    return _roi_align_levels_loop(fmaps, rois5, levels, scales, sampling_ratio, res)


# ------------------------------------------------------------------------------------ segmented top-k
TOPK_MAX_K = 4096                              # segmented_topk_*_kernel sorts at most this many elements in LDS
TopK = collections.namedtuple("TopK", "indices values offsets counts regression anchors")


def _stable_order(v):
    """Indices of a stable descending sort: NaN first, -0.0 == +0.0, ties by lower index."""
    return torch.sort(v, descending=True, stable=True).indices


def _segmented_topk_cpu(values, offsets, k, mask, global_index):
    out_off = _offsets(min(k, offsets[s + 1] - offsets[s]) for s in range(len(offsets) - 1))
    idx = torch.zeros(out_off[-1], dtype=torch.int32)
    val = torch.zeros(out_off[-1], dtype=torch.float32)
    counts = torch.zeros(len(offsets) - 1, dtype=torch.int32)
    for s in range(len(offsets) - 1):
        lo, hi = offsets[s], offsets[s + 1]
        seg = values[lo:hi]
        cand = torch.arange(hi - lo) if mask is None else torch.nonzero(mask[lo:hi]).reshape(-1)
        top = cand[_stable_order(seg[cand])[:k]]
        n = top.numel()
        idx[out_off[s]:out_off[s + 1]] = lo if global_index else 0
        idx[out_off[s]:out_off[s] + n] = (top + (lo if global_index else 0)).int()
        val[out_off[s]:out_off[s] + n] = seg[top]
        counts[s] = n
    return TopK(idx, val, out_off, counts if mask is not None else None, None, None)


def segmented_topk(values, offsets=None, k=1, mask=None, regression=None, anchors=None, global_index=False):
    """The first ``k`` (1 .. 4096) elements of every segment in the order of
    ``torch.sort(seg, descending=True, stable=True)``: NaN first, then larger values with ``-0.0 == +0.0``, ties by
    the lower index within the segment. One launch of csrc/detection.hip segmented_topk_*_kernel per 64 segments
    (flat) or for all segments (level maps), one workgroup per segment, any segment length below 2^31.

    Flat mode: ``values`` fp32 (R,), ``offsets`` the S + 1 monotone host offsets ending at R (empty segments
    allowed), ``mask`` an optional uint8 / bool (R,) whose zeros exclude elements. Level-map mode: ``values`` is a
    list of up to 8 objectness maps (N, A, H_l, W_l); segment (n, l) is image n of level l (image-major) and its
    element index is ``(h * W_l + w) * A + a``; ``regression`` (N, 4A, H_l, W_l) and ``anchors`` (H_l W_l A, 4) per
    level are gathered alongside.

    Returns TopK(indices int32, values, offsets, counts, regression, anchors): segment s owns the output slots
    ``offsets[s] : offsets[s] + min(k, len_s)`` in rank order; ``counts`` (int32 per segment, on the device) is given
    only with a mask, whose segment fills ``counts[s]`` slots, the rest holding the segment's first index and value
    0. Indices are relative to the segment, or into ``values`` with ``global_index`` (flat mode)."""
    k = int(k)
    assert 1 <= k <= TOPK_MAX_K, f"segmented_topk: k must be in 1 .. {TOPK_MAX_K}"
    if isinstance(values, (list, tuple)):
        obj = [o.float().contiguous() for o in values]
        reg = [r.float().contiguous() for r in regression]
        anc = [a.float().contiguous() for a in anchors]
        N = obj[0].shape[0]
        out_off = _offsets(min(k, o[0].numel()) for _ in range(N) for o in obj)
        dev, S = obj[0].device, out_off[-1]
        assert _on_gpu(obj[0]), "segmented_topk: the level-map mode runs on the GPU only"
        idx = torch.empty(S, dtype=torch.int32, device=dev)
        val = torch.empty(S, dtype=torch.float32, device=dev)
        greg = torch.empty(S, 4, dtype=torch.float32, device=dev)
        ganc = torch.empty(S, 4, dtype=torch.float32, device=dev)
        native.get().segmented_topk_maps(obj, reg, anc, k, idx, val, greg, ganc)
        return TopK(idx, val, out_off, None, greg, ganc)
    off = [int(o) for o in offsets]
    assert off[0] == 0 and off[-1] == values.numel(), "segmented_topk: offsets must start at 0 and end at R"
    if mask is not None:
        mask = mask.reshape(-1)
        mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    if not _on_gpu(values):
        return _segmented_topk_cpu(values.float(), off, k, mask, global_index)
    v = values.float().contiguous()
    out_off = _offsets(min(k, off[s + 1] - off[s]) for s in range(len(off) - 1))
    idx = torch.empty(out_off[-1], dtype=torch.int32, device=v.device)
    val = torch.empty(out_off[-1], dtype=torch.float32, device=v.device)
    counts = None if mask is None else torch.empty(len(off) - 1, dtype=torch.int32, device=v.device)
    native.get().segmented_topk_flat(v, None if mask is None else mask.contiguous(), off, out_off, k,
                                     bool(global_index), idx, val, counts)
    return TopK(idx, val, out_off, counts, None, None)


# ------------------------------------------------------------------------------------------ RPN selection
def _rpn_clip(props, im_size):
    """clip_boxes of (K, 4) proposals to im_size = (height, width); a device tensor is not read back."""
    if torch.is_tensor(im_size) and _on_gpu(im_size):
        hw = im_size.reshape(-1).float()
        props[:, 0::2] = torch.minimum(props[:, 0::2].clamp_min(0), hw[1] - 1)
        props[:, 1::2] = torch.minimum(props[:, 1::2].clamp_min(0), hw[0] - 1)
        return props
    hw = im_size.reshape(-1) if torch.is_tensor(im_size) else im_size
    clip_boxes(props, float(hw[0]), float(hw[1]))
    return props


def _rpn_select_loop(objectness, regression, anchors, im_size, pre_topk, post_topk, nms_thresh):
    out = []
    for b in range(objectness[0].shape[0]):
        boxes, logits = [], []
        for obj, reg, anc in zip(objectness, regression, anchors):
            _, A, H, W = obj.shape
            o = obj[b].float().permute(1, 2, 0).reshape(-1)                               # (h, w, a)
            r = reg[b].float().reshape(A, 4, H, W).permute(2, 3, 0, 1).reshape(-1, 4)
            order = _stable_order(o)[:pre_topk]
            props = _rpn_clip(bbox_transform_inv(anc.to(r.device).float()[order], r[order], normalized=True), im_size)
            keep = nms_sorted(props, nms_thresh)
            boxes.append(props[keep])
            logits.append(o[order][keep])
        allb, alls = torch.cat(boxes), torch.cat(logits)
        out.append(allb[_stable_order(alls)[:post_topk]])
    return out


def rpn_nms_launch(props, offsets, nms_thresh):
    """Greedy NMS (pixel ``+1`` areas) of ranked boxes: props fp32 (R, 4) on the GPU, every segment
    ``offsets[s] : offsets[s + 1]`` (at most 4096 rows, fewer than 2^24 rows in all) already in rank order. One
    nms_classes_kernel launch with C = Cb = 1 and a descending ramp as scores, so the kernel's own sort keeps the
    rank order whatever the values the ranking came from (NaN included). Returns the uint8 (R,) keep mask."""
    R = props.shape[0]
    assert R < (1 << 24) and all(b - a <= TOPK_MAX_K for a, b in zip(offsets, offsets[1:]))
    ramp = torch.arange(R, 0, -1, dtype=torch.float32, device=props.device).reshape(R, 1)
    keep = torch.empty(R, 1, dtype=torch.uint8, device=props.device)
    overflow = torch.empty(1, dtype=torch.int32, device=props.device)   # a segment fits the capacity: never set
    nms_classes_launch(ramp, props.float().contiguous().reshape(R, 1, 4), offsets, 0.0, nms_thresh, -1, True, -1,
                       False, keep, overflow)
    return keep.reshape(R)


def rpn_select(objectness, regression, anchors, im_size, pre_topk, post_topk, nms_thresh):
    """FPN proposal selection for a whole batch. Per level l: ``objectness[l]`` (N, A, H_l, W_l) raw logits,
    ``regression[l]`` (N, 4A, H_l, W_l), ``anchors[l]`` (H_l W_l A, 4) in (h, w, a) order; ``im_size`` = (height,
    width). Per image and level the ``pre_topk`` best anchors are decoded (``bbox_transform_inv(normalized=True)``),
    clipped and suppressed greedily at ``nms_thresh`` (pixel ``+1`` areas); the ``post_topk`` best survivors of all
    levels of an image are its proposals. Returns the list of per-image (K_n, 4) boxes.

    Ranking is on the logits, in the order of ``segmented_topk``: a stable descending sort, ties by lower anchor
    index, then by level. ``RegionProposal``'s per-image loop ranks ``sigmoid(logit)`` with ``torch.topk``; sigmoid
    is monotone, so the two agree wherever fp32 sigmoid keeps the values apart, and where it collapses them (it
    saturates near 1) the loop's order is ``torch.topk``'s unspecified tie order, which this op replaces by the
    defined one. Only boxes are returned, so no sigmoid is evaluated.

    On the GPU with batching on (at most 8 levels, ``pre_topk`` / ``post_topk`` at most 4096) this is one level-map
    ``segmented_topk`` launch, one decode, one ``nms_classes_kernel`` launch with a segment per (image, level) and a
    descending ramp as scores, one flat ``segmented_topk`` launch over the kept rows, one read of the per-image
    counts (the only synchronisation) and one gather. Otherwise the same pipeline runs segment by segment with
    ``torch.sort(stable=True)`` and ``nms_sorted``; the two forms are bit-equal."""
    objectness, regression, anchors = list(objectness), list(regression), list(anchors)
    L, N = len(objectness), objectness[0].shape[0]
    pre_topk, post_topk = int(pre_topk), int(post_topk)
    assert L == len(regression) == len(anchors) and pre_topk >= 1 and post_topk >= 1
    if not (batched(_on_gpu(objectness[0])) and L <= 8 and pre_topk <= TOPK_MAX_K and post_topk <= TOPK_MAX_K
            and N * L < 4096):                               # rpn_nms_launch: fewer than 2^24 rows
        _set_route("rpn_select", "loop")
        return _rpn_select_loop(objectness, regression, anchors, im_size, pre_topk, post_topk, nms_thresh)
    dev = objectness[0].device
    top = segmented_topk(objectness, k=pre_topk, regression=regression, anchors=[a.to(dev) for a in anchors])
    props = _rpn_clip(bbox_transform_inv(top.anchors, top.regression, normalized=True), im_size)
    keep = rpn_nms_launch(props, top.offsets, nms_thresh)
    fin = segmented_topk(top.values, top.offsets[::L], post_topk, mask=keep, global_index=True)
    counts = fin.counts.tolist()
    rows = props[fin.indices.long()]
    _set_route("rpn_select", "batched")
    return [rows[fin.offsets[b]:fin.offsets[b] + counts[b]] for b in range(N)]


# ------------------------------------------------------------------------------------------- RoiAlign
def roi_align(x, rois, spatial_scale, sampling_ratio, pooled_h, pooled_w):
    """x: (N, C, H, W); rois: (R, 4) boxes of image 0 (reference) or (R, 5) (batch, x1, y1, x2, y2)."""
    R, C = rois.shape[0], x.shape[1]
    if _on_gpu(x):
        out = torch.empty(R, C, pooled_h, pooled_w, dtype=torch.float32, device=x.device)
        if R:
            native.get().roi_align_fwd(x.float().contiguous(), rois.float().contiguous(), out, float(spatial_scale),
                                       int(sampling_ratio))
        return out
    return _roi_align_cpu(x.float(), rois.float(), spatial_scale, sampling_ratio, pooled_h, pooled_w)


def _roi_align_cpu(x, rois, scale, sampling, PH, PW):
    N, C, H, W = x.shape
    R = rois.shape[0]
    out = torch.zeros(R, C, PH, PW)
    f32 = np.float32
    for r in range(R):
        roi = rois[r].tolist()
        b = int(roi[0]) if len(roi) == 5 else 0
        x1, y1, x2, y2 = [f32(v) * f32(scale) for v in (roi[-4:])]
        rw, rh = max(x2 - x1, f32(1.0)), max(y2 - y1, f32(1.0))
        bh, bw = f32(rh / f32(PH)), f32(rw / f32(PW))
        gh = sampling if sampling > 0 else int(math.ceil(rh / PH))
        gw = sampling if sampling > 0 else int(math.ceil(rw / PW))
        # sampling positions of the whole (PH * gh) x (PW * gw) grid
        iy = np.arange(PH * gh)
        ys = (y1 + (iy // gh).astype(f32) * bh + ((iy % gh).astype(f32) + f32(0.5)) * bh / f32(gh)).astype(f32)
        ix = np.arange(PW * gw)
        xs = (x1 + (ix // gw).astype(f32) * bw + ((ix % gw).astype(f32) + f32(0.5)) * bw / f32(gw)).astype(f32)

        def axis(v, size):
            valid = (v >= -1.0) & (v <= size)
            v = np.maximum(v, 0)
            lo = v.astype(np.int64)
            edge = lo >= size - 1
            lo = np.where(edge, size - 1, lo)
            hi = np.where(edge, lo, lo + 1)
            v = np.where(edge, lo.astype(f32), v)
            l = (v - lo).astype(f32)
            return valid, lo, hi, l

        vy, yl, yh, ly = axis(ys, H)
        vx, xl, xh, lx = axis(xs, W)
        img = x[b]
        wy_l = torch.as_tensor((1 - ly) * vy, dtype=torch.float32)
        wy_h = torch.as_tensor(ly * vy, dtype=torch.float32)
        wx_l = torch.as_tensor((1 - lx) * vx, dtype=torch.float32)
        wx_h = torch.as_tensor(lx * vx, dtype=torch.float32)
        yl_t, yh_t = torch.as_tensor(yl), torch.as_tensor(yh)
        xl_t, xh_t = torch.as_tensor(xl), torch.as_tensor(xh)
        # separable bilinear: rows then columns
        rows = img[:, yl_t, :] * wy_l[None, :, None] + img[:, yh_t, :] * wy_h[None, :, None]   # C, PH*gh, W
        val = rows[:, :, xl_t] * wx_l[None, None, :] + rows[:, :, xh_t] * wx_h[None, None, :]  # C, PH*gh, PW*gw
        out[r] = val.reshape(C, PH, gh, PW, gw).sum(dim=(2, 4)) / float(gh * gw)
    return out


# ----------------------------------------------------------------------------------------- RoiPooling
def _jround(v):
    return int(math.floor(v + 0.5))          # Java Math.round


def roi_pool_forward(x, rois, spatial_scale, PH, PW):
    """Returns (out (R, C, PH, PW), argmax int32 (flat h*W+w within the map, -1 for empty bins))."""
    R, C = rois.shape[0], x.shape[1]
    if _on_gpu(x):
        out = torch.empty(R, C, PH, PW, dtype=torch.float32, device=x.device)
        arg = torch.empty(R, C, PH, PW, dtype=torch.int32, device=x.device)
        if R:
            native.get().roi_pool_fwd(x.float().contiguous(), rois.float().contiguous(), out, arg,
                                      float(spatial_scale))
        return out, arg
    x = x.float()
    H, W = x.shape[2], x.shape[3]
    out = torch.zeros(R, C, PH, PW)
    arg = torch.full((R, C, PH, PW), -1, dtype=torch.int32)
    for r in range(R):
        b, rx1, ry1, rx2, ry2 = rois[r].tolist()
        sw, sh = _jround(np.float32(rx1) * np.float32(spatial_scale)), _jround(np.float32(ry1) * np.float32(spatial_scale))
        ew, eh = _jround(np.float32(rx2) * np.float32(spatial_scale)), _jround(np.float32(ry2) * np.float32(spatial_scale))
        bh = np.float32(max(eh - sh + 1, 1)) / np.float32(PH)
        bw = np.float32(max(ew - sw + 1, 1)) / np.float32(PW)
        fmap = x[int(b)].reshape(C, H * W)
        for ph in range(PH):
            hs = min(max(int(math.floor(ph * bh)) + sh, 0), H)
            he = min(max(int(math.ceil((ph + 1) * bh)) + sh, 0), H)
            for pw in range(PW):
                ws = min(max(int(math.floor(pw * bw)) + sw, 0), W)
                we = min(max(int(math.ceil((pw + 1) * bw)) + sw, 0), W)
                if he <= hs or we <= ws:
                    continue
                idx = (torch.arange(hs, he)[:, None] * W + torch.arange(ws, we)[None, :]).reshape(-1)
                vals = fmap[:, idx]
                m, a = vals.max(dim=1)
                out[r, :, ph, pw] = m
                arg[r, :, ph, pw] = idx[a].int()
    return out, arg


def roi_pool_backward(gy, argmax, rois, x_shape):
    gx = torch.zeros(x_shape, dtype=torch.float32, device=gy.device)
    if _on_gpu(gy):
        native.get().roi_pool_bwd(gy.float().contiguous(), argmax.contiguous(), rois.float().contiguous(), gx)
        return gx
    N, C, H, W = x_shape
    R = gy.shape[0]
    b = rois[:, 0].long()
    flat = gx.reshape(N, C, H * W)
    a = argmax.reshape(R, C, -1).long()
    g = gy.reshape(R, C, -1).float()
    valid = a >= 0
    for r in range(R):
        flat[b[r]].scatter_add_(1, a[r].clamp(min=0), g[r] * valid[r])
    return gx


# ------------------------------------------------------------------------------------------- BboxUtil
def bbox_transform_inv(boxes, deltas, normalized=False):
    """Reference BboxUtil.bboxTransformInv: boxes (N, 4), deltas (N, 4a) -> decoded (N, 4a)."""
    if boxes.shape[0] == 0:
        return boxes.clone()
    one = 0.0 if normalized else 1.0
    w = (boxes[:, 2] - boxes[:, 0] + one)[:, None]
    h = (boxes[:, 3] - boxes[:, 1] + one)[:, None]
    x1, y1 = boxes[:, 0:1], boxes[:, 1:2]
    d = deltas.reshape(deltas.shape[0], -1, 4)
    cx = d[..., 0] * w + x1 + w / 2
    cy = d[..., 1] * h + y1 + h / 2
    pw = torch.exp(d[..., 2]) * w / 2
    ph = torch.exp(d[..., 3]) * h / 2
    return torch.stack([cx - pw, cy - ph, cx + pw, cy + ph], dim=-1).reshape(deltas.shape)


def clip_boxes(boxes, height, width, min_h=0.0, min_w=0.0, scores=None):
    """In-place clip of (N, 4a) pixel boxes to the image; zero the scores of boxes smaller than min_h/min_w.
    Returns the number of boxes that pass the size test (reference BboxUtil.clipBoxes)."""
    b = boxes.view(boxes.shape[0], -1, 4)
    b[..., 0::2].clamp_(0, width - 1)
    b[..., 1::2].clamp_(0, height - 1)
    if scores is None:
        return boxes.shape[0]
    ws = b[..., 2] - b[..., 0] + 1
    hs = b[..., 3] - b[..., 1] + 1
    small = ((ws < min_w) | (hs < min_h)).reshape(-1)
    sc = scores.view(-1)
    sc[small] = 0
    return int((~small).sum())


def clip_normalized(boxes):
    return boxes.clamp_(0, 1)


def scale_bbox(boxes, height, width):
    if boxes.numel():
        boxes[:, 0::2] *= width
        boxes[:, 1::2] *= height
    return boxes


def decode_with_weight(encoded, boxes, weight=(10.0, 10.0, 5.0, 5.0), bbox_clip=62.5):
    """Reference BboxUtil.decodeWithWeight (Detectron-style deltas with weights; w/h clamped from above)."""
    wdt = boxes[:, 2] - boxes[:, 0] + 1
    hgt = boxes[:, 3] - boxes[:, 1] + 1
    cx = boxes[:, 0] + wdt / 2
    cy = boxes[:, 1] + hgt / 2
    d = encoded.reshape(encoded.shape[0], -1, 4)
    dx, dy = d[..., 0] / weight[0], d[..., 1] / weight[1]
    dw = torch.clamp(d[..., 2] / weight[2], max=bbox_clip)
    dh = torch.clamp(d[..., 3] / weight[3], max=bbox_clip)
    pcx = dx * wdt[:, None] + cx[:, None]
    pcy = dy * hgt[:, None] + cy[:, None]
    pw = torch.exp(dw) * wdt[:, None] * 0.5
    ph = torch.exp(dh) * hgt[:, None] * 0.5
    return torch.stack([pcx - pw, pcy - ph, pcx + pw - 1, pcy + ph - 1], dim=-1).reshape(encoded.shape)


def decode_boxes(prior_boxes, prior_variances, clip, bboxes, variance_encoded_in_target=False):
    """SSD decode (reference BboxUtil.decodeBoxes / decodeSingleBbox)."""
    pw = prior_boxes[:, 2] - prior_boxes[:, 0]
    ph = prior_boxes[:, 3] - prior_boxes[:, 1]
    pcx = (prior_boxes[:, 0] + prior_boxes[:, 2]) / 2
    pcy = (prior_boxes[:, 1] + prior_boxes[:, 3]) / 2
    v = torch.ones_like(prior_variances) if variance_encoded_in_target else prior_variances
    cx = v[:, 0] * bboxes[:, 0] * pw + pcx
    cy = v[:, 1] * bboxes[:, 1] * ph + pcy
    w = torch.exp(v[:, 2] * bboxes[:, 2]) * pw
    h = torch.exp(v[:, 3] * bboxes[:, 3]) * ph
    out = torch.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], dim=1)
    return out.clamp_(0, 1) if clip else out


def bbox_areas(boxes, normalized=False):
    one = 0.0 if normalized else 1.0
    return (boxes[:, 2] - boxes[:, 0] + one) * (boxes[:, 3] - boxes[:, 1] + one)


def bbox_vote(scores_nms, bbox_nms, scores_all, bbox_all):
    """Reference BboxUtil.bboxVote: replace each kept box by the score-weighted mean of all boxes that overlap
    it with IoU >= 0.5."""
    a_all = bbox_areas(bbox_all)
    out = bbox_nms.clone()
    for i in range(bbox_nms.shape[0]):
        b = bbox_nms[i]
        iw = torch.minimum(b[2], bbox_all[:, 2]) - torch.maximum(b[0], bbox_all[:, 0]) + 1
        ih = torch.minimum(b[3], bbox_all[:, 3]) - torch.maximum(b[1], bbox_all[:, 1]) + 1
        inter = iw * ih
        ua = (b[2] - b[0] + 1) * (b[3] - b[1] + 1) + a_all - inter
        sel = (iw > 0) & (ih > 0) & (inter / ua >= 0.5)
        w = scores_all.reshape(-1) * sel
        out[i] = (w[:, None] * bbox_all).sum(0) / w.sum()
    return scores_nms, out


def decode_rois(output):
    """Reference BboxUtil.decodeRois: flat detection output [num, (label, score, x1, y1, x2, y2)*] -> (num, 6)."""
    if output.numel() < 6 or output.dim() == 2:
        return output
    num = int(output.reshape(-1)[0].item())
    if num == 0:
        return output.new_zeros(0, 6)
    return output.reshape(-1)[1: 1 + num * 6].view(num, 6)
