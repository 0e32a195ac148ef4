"""Shared inputs and the integer oracle of the batched detection tests (test_detection_batched_{cpu,gpu}.py).

Oracle inputs: integer pixel boxes with corner in [0, 64) and side in [8, 56), so every coordinate is an integer in
[0, 119] and every ``+1`` area is at most 56 * 56 < 2^13; scores are multiples of 1/32, so ties are frequent. At
NMS threshold 0.5 the suppression test ``inter / union > 0.5`` is ``2 * inter > union`` on integers: when it holds
the quotient is at least 0.5 + 1 / (2 * union) > 0.5 + 2^-15, when it fails the quotient is at most 0.5 exactly, so
an fp32 division decides every pair the way the integers do and the oracle is exact for the CPU and the GPU paths.
"""
import torch

NMS_THRESH = 0.5
SCORE_STEPS = 32


def int_inputs(counts, C, Cb, seed):
    """scores (R, C) multiples of 1/32 in [0, 1]; boxes (R, Cb, 4) integer-valued fp32."""
    g = torch.Generator().manual_seed(seed)
    R = sum(counts)
    xy = torch.randint(0, 64, (R, Cb, 2), generator=g)
    wh = torch.randint(8, 56, (R, Cb, 2), generator=g)
    boxes = torch.cat([xy, xy + wh], 2).float()
    scores = torch.randint(0, SCORE_STEPS + 1, (R, C), generator=g).float() / SCORE_STEPS
    return scores, boxes


def float_inputs(counts, C, Cb, seed, normalized=False):
    """Gaussian float boxes around a few centres (so many overlap) and uniform scores."""
    g = torch.Generator().manual_seed(seed)
    R = sum(counts)
    ctr = torch.randn(R, Cb, 2, generator=g) * 40 + 200
    half = torch.randn(R, Cb, 2, generator=g).abs() * 25 + 10
    boxes = torch.cat([ctr - half, ctr + half], 2)
    if normalized:
        boxes = boxes / 400.0
    scores = torch.rand(R, C, generator=g)
    return scores, boxes


def _suppresses(a, b):
    """Integer form of iou_gt at threshold 0.5 with ``+1`` pixel areas."""
    w = min(a[2], b[2]) - max(a[0], b[0]) + 1
    h = min(a[3], b[3]) - max(a[1], b[1]) + 1
    if w < 0 or h < 0:
        return False
    inter = w * h
    union = (a[2] - a[0] + 1) * (a[3] - a[1] + 1) + (b[2] - b[0] + 1) * (b[3] - b[1] + 1) - inter
    return 2 * inter > union


def oracle_segment(score32, boxes, thresh32, inclusive=False, pre_topk=-1):
    """Kept rows (a set) of one segment. score32 / thresh32 are the scores times 32 as ints, boxes int 4-tuples."""
    cand = [r for r, s in enumerate(score32) if (s >= thresh32 if inclusive else s > thresh32)]
    cand.sort(key=lambda r: (-score32[r], r))
    if pre_topk > 0:
        cand = cand[:pre_topk]
    kept = []
    for r in cand:
        if not any(_suppresses(boxes[k], boxes[r]) for k in kept):
            kept.append(r)
    return set(kept)


def oracle_mask(scores, boxes, counts, thresh32, skip_class=0, inclusive=False, pre_topk=-1):
    """The (R, C) bool mask the oracle gives for integer inputs from ``int_inputs``."""
    R, C = scores.shape
    Cb = boxes.shape[1]
    s32 = (scores * SCORE_STEPS).round().long().tolist()
    bi = boxes.long().tolist()
    mask = torch.zeros(R, C, dtype=torch.bool)
    lo = 0
    for n in counts:
        for c in range(C):
            if c == skip_class:
                continue
            cb = c if Cb > 1 else 0
            kept = oracle_segment([s32[lo + r][c] for r in range(n)], [bi[lo + r][cb] for r in range(n)], thresh32,
                                  inclusive, pre_topk)
            for r in kept:
                mask[lo + r, c] = True
        lo += n
    return mask


def table_tensors(out):
    """Every tensor of a module output (Tensor or nested Table), depth first in key order."""
    if isinstance(out, torch.Tensor):
        return [out]
    res = []
    for i in range(out.length()):
        res += table_tensors(out[i + 1])
    return res


def box_post_inputs(counts, C, seed, tie=False):
    """(logits, deltas, proposals Table, info) for BoxPostProcessor."""
    from bigdl_amd.utils.table import Table

    g = torch.Generator().manual_seed(seed)
    R = sum(counts)
    logits = torch.randn(R, C, generator=g) * 2
    if tie:                       # equal logit rows give equal softmax rows: ties at any cut
        logits[1::2] = logits[0::2][: logits[1::2].shape[0]]
    deltas = torch.randn(R, 4 * C, generator=g) * 0.3
    ctr = torch.randn(R, 2, generator=g) * 20 + 60
    half = torch.rand(R, 2, generator=g) * 20 + 6
    props = torch.cat([ctr - half, ctr + half], 1)
    tab, lo = Table(), 0
    for i, n in enumerate(counts):
        tab[i + 1] = props[lo:lo + n]
        lo += n
    return logits, deltas, tab, torch.tensor([128.0, 160.0])


def ssd_inputs(B, C, share, seed):
    from bigdl_amd import nn

    g = torch.Generator().manual_seed(seed)
    prior = nn.PriorBox([30.0], [60.0], [2.0], variances=[0.1, 0.1, 0.2, 0.2], imgH=300, imgW=300).forward(
        torch.zeros(1, 4, 3, 2))
    npri = prior.shape[2] // 4
    nl = 1 if share else C
    loc = torch.randn(B, npri * nl * 4, generator=g) * 0.1
    conf = torch.randn(B, npri * C, generator=g)
    return loc, conf, prior


def frcnn_inputs(R, C, seed):
    g = torch.Generator().manual_seed(seed)
    ctr = torch.randn(R, 2, generator=g) * 25 + 100
    half = torch.rand(R, 2, generator=g) * 25 + 8
    rois = torch.cat([torch.zeros(R, 1), ctr - half, ctr + half], 1)
    scores = torch.softmax(torch.randn(R, C, generator=g) * 2, 1)
    deltas = torch.randn(R, 4 * C, generator=g) * 0.2
    return torch.tensor([[200.0, 200.0, 1.0, 1.0]]), rois, deltas, scores
