"""Shared inputs and the pure-Python oracles of the batched region-proposal tests (test_rpn_batched_{cpu,gpu}.py).

The order under test is that of ``torch.sort(descending=True, stable=True)``: NaN first (all NaNs equal), then larger
values with ``-0.0 == +0.0``, ties by the lower index. ``oracle_topk`` spells it as a Python sort key.
"""
import math

import torch

# the segment lengths of one flat call: empty, one element, around the wave, the workgroup (1024) and the LDS
# capacity (4096), two workgroup strides past it, and the length of a 120 x 200 x 3 pyramid level
FLAT_LENGTHS = [0, 1, 255, 256, 257, 1023, 1025, 4097, 8193, 72000]
KS = [1, 50, 1000, 4096]
SPECIAL = [0.0, -0.0, float("nan"), 1.0, float("inf"), float("nan"), float("-inf"), 0.0, 1.0]
SPECIAL_ORDER = [2, 5, 4, 3, 8, 0, 1, 7, 6]


def oracle_topk(values, k, mask=None):
    """values: a list of Python floats; mask: a list of 0 / 1 or None. The first k indices of the order."""
    idx = [i for i in range(len(values)) if mask is None or mask[i]]
    idx.sort(key=lambda i: (0, 0.0, i) if math.isnan(values[i]) else (1, -values[i], i))
    return idx[:k]


def offsets(lengths):
    off = [0]
    for n in lengths:
        off.append(off[-1] + n)
    return off


def uniform_values(n, seed):
    return torch.rand(n, generator=torch.Generator().manual_seed(seed)) * 8 - 4


def quantised_values(n, seed):
    """Multiples of 1/8 in [-4, 4]: 65 distinct values, so long runs of ties."""
    return torch.randint(-32, 33, (n,), generator=torch.Generator().manual_seed(seed)).float() / 8


def special_values(n, seed):
    """Uniform floats with NaN, +/-inf and +/-0.0 mixed in at random places (about one element in four)."""
    g = torch.Generator().manual_seed(seed)
    v = torch.rand(n, generator=g) * 2 - 1
    pick = torch.randint(0, 20, (n,), generator=g)
    for code, x in enumerate([float("nan"), float("inf"), float("-inf"), 0.0, -0.0]):
        v[pick == code] = x
    return v


def check_flat(result, values, off, k, mask=None):
    """Assert that a TopK of flat mode equals the oracle on every segment; only slots below the count are read."""
    idx, val = result.indices.cpu(), result.values.cpu()
    counts = None if result.counts is None else result.counts.cpu().tolist()
    vals, m = values.tolist(), None if mask is None else mask.tolist()
    assert len(result.offsets) == len(off)
    for s in range(len(off) - 1):
        lo, hi = off[s], off[s + 1]
        want = oracle_topk(vals[lo:hi], k, None if m is None else m[lo:hi])
        o = result.offsets[s]
        assert result.offsets[s + 1] - o == min(k, hi - lo)
        if counts is not None:
            assert counts[s] == len(want), f"segment {s}: count {counts[s]} != {len(want)}"
        else:
            assert len(want) == min(k, hi - lo)
        assert idx[o:o + len(want)].tolist() == want, f"segment {s} (length {hi - lo}, k {k})"
        got = val[o:o + len(want)]
        ref = values[lo:hi][torch.tensor(want, dtype=torch.long)]
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), f"segment {s}: values"


# ------------------------------------------------------------------------------------------------- RPN inputs
def anchors_for(sizes, ratios, strides, shapes):
    """The real Anchor tables of the levels: (H_l W_l A, 4) in (h, w, a) order."""
    from bigdl_amd.nn.detection import Anchor

    return [Anchor(ratios, [s / st]).generateAnchors(w, h, st) for s, st, (h, w) in zip(sizes, strides, shapes)]


def rpn_inputs(N, shapes, A, seed, reg_scale=0.3):
    """Per-level objectness (N, A, H, W) logits and regression (N, 4A, H, W)."""
    g = torch.Generator().manual_seed(seed)
    obj = [torch.randn(N, A, h, w, generator=g) * 2 for h, w in shapes]
    reg = [torch.randn(N, 4 * A, h, w, generator=g) * reg_scale for h, w in shapes]
    return obj, reg


def _iou_gt(a, b, thresh):
    w = min(a[2], b[2]) - max(a[0], b[0]) + 1.0
    h = min(a[3], b[3]) - max(a[1], b[1]) + 1.0
    if w < 0 or h < 0:
        return False
    inter = w * h
    union = (a[2] - a[0] + 1.0) * (a[3] - a[1] + 1.0) + (b[2] - b[0] + 1.0) * (b[3] - b[1] + 1.0) - inter
    return inter / union > thresh


def oracle_rpn(obj, reg, anchors, im_size, pre_topk, post_topk, thresh):
    """The pipeline of rpn_select with Python sorts and a Python greedy NMS in double precision (as the CPU
    ``nms_sorted``); decode and clip are the project's element-wise torch functions. Returns (boxes per image,
    [(candidates, kept) per (image, level)])."""
    from bigdl_amd.ops import detection as D

    out, stages = [], []
    for b in range(obj[0].shape[0]):
        boxes, logits = [], []
        for o, r, anc in zip(obj, reg, anchors):
            _, A, H, W = o.shape
            flat = o[b].permute(1, 2, 0).reshape(-1)
            rows = r[b].reshape(A, 4, H, W).permute(2, 3, 0, 1).reshape(-1, 4)
            order = torch.tensor(oracle_topk(flat.tolist(), pre_topk), dtype=torch.long)
            props = D.bbox_transform_inv(anc[order], rows[order], normalized=True)
            D.clip_boxes(props, float(im_size[0]), float(im_size[1]))
            pl, kept = props.double().tolist(), []
            for i in range(len(pl)):
                if not any(_iou_gt(pl[j], pl[i], thresh) for j in kept):
                    kept.append(i)
            stages.append((len(pl), len(kept)))
            boxes.append(props[kept])
            logits += flat[order][kept].tolist()
        allb = torch.cat(boxes)
        out.append(allb[torch.tensor(oracle_topk(logits, post_topk), dtype=torch.long)])
    return out, stages


def slice_head(A):
    """Stands in for the RPN head: objectness = the first A channels of the feature map, regression = the next 4A,
    so every route sees the same bits whatever the batch size."""
    from bigdl_amd.nn.abstractnn import AbstractModule
    from bigdl_amd.utils.table import Table

    class SliceHead(AbstractModule):
        def updateOutput(self, x):
            return Table(x[:, :A], x[:, A:5 * A])

    return SliceHead()


MODULE_SHAPES = [(16, 16), (8, 8), (4, 4)]


def module_case(N, seed):
    """(RegionProposal with the slicing head, features Table (N, 15, H_l, W_l), image size): the logits of an image
    are a random permutation of the grid ``-6 + i / 1024`` over all its anchors, whose fp32 sigmoids are distinct."""
    from bigdl_amd import nn
    from bigdl_amd.utils.table import Table

    g = torch.Generator().manual_seed(seed)
    rp = nn.RegionProposal(15, [32, 64, 128], [0.5, 1, 2], [4, 8, 16], 50, 20, 50, 20).evaluate()
    rp.head = slice_head(3)
    rp.modules = [rp.head]
    per_level = [3 * h * w for h, w in MODULE_SHAPES]
    total = sum(per_level)
    feats = [torch.randn(N, 15, h, w, generator=g) * 0.3 for h, w in MODULE_SHAPES]
    for b in range(N):
        grid = (-6 + torch.arange(total, dtype=torch.float32) / 1024)[torch.randperm(total, generator=g)]
        lo = 0
        for f, n, (h, w) in zip(feats, per_level, MODULE_SHAPES):
            f[b, :3] = grid[lo:lo + n].reshape(3, h, w)
            lo += n
    tab = Table()
    for i, f in enumerate(feats):
        tab[i + 1] = f
    return rp, tab, torch.tensor([64.0, 64.0])


def module_logits(tab, b):
    return torch.cat([tab[i + 1][b, :3].reshape(-1) for i in range(tab.length())])
