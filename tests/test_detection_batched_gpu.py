"""nms_classes_kernel / roi_align_levels_fwd_kernel (csrc/detection.hip) and the modules that use them, on the GPU:
masks against the integer oracle and the per-class loop, bit-equal RoiAlign against the per-level path, module
outputs batched against loop, the overflow fall-back and a HIP-graph replay (GPU only)."""
import json
import os

import pytest
import torch

from bigdl_amd import nn
from bigdl_amd.ops import detection as D
from bigdl_amd.utils.table import T
from tests import detection_batched_cases as dc

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(__file__), "fixtures", "detection")

# rows per image, C, Cb, skip_class
CASES = [([1], 3, 3, 0), ([63], 3, 3, 0), ([64], 3, 1, -1), ([65], 3, 3, -1), ([129], 3, 1, 0), ([300], 3, 3, 0),
         ([0, 65, 7], 3, 3, 0), ([0, 65, 7], 3, 1, -1), ([130], 81, 81, 0), ([1030], 2, 2, -1)]
_IDS = ["-".join(map(str, c[0])) + f"_C{c[1]}_Cb{c[2]}_skip{c[3]}" for c in CASES]


@pytest.fixture(autouse=True)
def _default_switch():
    D.set_batched(None)
    yield
    D.set_batched(None)


def _batched(scores, boxes, counts, *a, **kw):
    got = D.multiclass_nms(scores.cuda(), boxes.cuda(), counts, *a, **kw)
    assert D.last_route("multiclass_nms") == "batched" and D.last_route() == "batched"
    assert got.dtype == torch.bool and tuple(got.shape) == tuple(scores.shape)
    return got.cpu()


def _loop(scores, boxes, counts, *a, **kw):
    D.set_batched(False)
    try:
        got = D.multiclass_nms(scores.cuda(), boxes.cuda(), counts, *a, **kw)
        assert D.last_route("multiclass_nms") == "loop"
    finally:
        D.set_batched(None)
    return got.cpu()


# ------------------------------------------------------------------------------------------- the mask
@pytest.mark.parametrize("counts,C,Cb,skip", CASES, ids=_IDS)
def test_mask_equals_integer_oracle(counts, C, Cb, skip):
    scores, boxes = dc.int_inputs(counts, C, Cb, seed=sum(counts) + C)
    got = _batched(scores, boxes, counts, 0.25, dc.NMS_THRESH, skip_class=skip)
    assert torch.equal(got, dc.oracle_mask(scores, boxes, counts, 8, skip))


@pytest.mark.parametrize("counts,C,Cb,skip", CASES, ids=_IDS)
def test_mask_equals_gpu_loop_on_float_boxes(counts, C, Cb, skip):
    scores, boxes = dc.float_inputs(counts, C, Cb, seed=sum(counts) + C + 1)
    got = _batched(scores, boxes, counts, 0.3, 0.45, skip_class=skip)
    ref = _loop(scores, boxes, counts, 0.3, 0.45, skip_class=skip)
    assert torch.equal(got, ref)
    if sum(counts) >= 63:
        live = [c for c in range(C) if c != skip]
        cand = int((scores[:, live] > 0.3).sum())
        assert 0 < int(got.sum()) < cand          # the case both keeps and suppresses


@pytest.mark.parametrize("rows,cap", [(256, 256), (257, 1024), (1024, 1024), (1025, 4096)])
def test_capacity_follows_longest_image(rows, cap):
    scores, boxes = dc.int_inputs([3, rows], 1, 1, seed=rows)
    keep = torch.empty(rows + 3, 1, dtype=torch.uint8, device="cuda")
    ov = torch.empty(1, dtype=torch.int32, device="cuda")
    assert D.nms_classes_launch(scores.cuda(), boxes.cuda(), [0, 3, rows + 3], -1.0, 0.5, -1, False, -1, False, keep,
                                ov) == cap
    assert int(ov.item()) == 0
    assert torch.equal(keep.bool().cpu(), dc.oracle_mask(scores, boxes, [3, rows], -32, -1))


@pytest.mark.parametrize("inclusive", [False, True])
def test_scores_exactly_at_the_threshold(inclusive):
    scores, boxes = dc.int_inputs([129], 3, 3, seed=11)
    assert int((scores == 0.25).sum()) > 0
    got = _batched(scores, boxes, [129], 0.25, dc.NMS_THRESH, skip_class=-1, inclusive=inclusive)
    assert torch.equal(got, dc.oracle_mask(scores, boxes, [129], 8, -1, inclusive))
    assert bool(got[scores == 0.25].any()) == inclusive
    assert torch.equal(got, _loop(scores, boxes, [129], 0.25, dc.NMS_THRESH, skip_class=-1, inclusive=inclusive))


@pytest.mark.parametrize("topk", [10, 1000])
def test_pre_topk(topk):
    scores, boxes = dc.int_inputs([48], 2, 1, seed=12)
    cand = (scores >= 5 / 32).sum(0)
    assert 30 <= int(cand.min()) and int(cand.max()) <= 48
    got = _batched(scores, boxes, [48], 5 / 32, dc.NMS_THRESH, skip_class=-1, inclusive=True, pre_topk=topk)
    assert torch.equal(got, dc.oracle_mask(scores, boxes, [48], 5, -1, True, topk))
    assert torch.equal(got, _loop(scores, boxes, [48], 5 / 32, dc.NMS_THRESH, skip_class=-1, inclusive=True,
                                  pre_topk=topk))
    if topk == 10:
        assert int(got.sum(0).max()) <= 10


def test_normalized_boxes():
    scores, boxes = dc.float_inputs([65, 40], 3, 1, seed=13, normalized=True)
    kw = dict(skip_class=0, inclusive=True, pre_topk=50, normalized=True)
    got = _batched(scores, boxes, [65, 40], 0.2, 0.45, **kw)
    assert torch.equal(got, _loop(scores, boxes, [65, 40], 0.2, 0.45, **kw))
    # the +1 of pixel boxes matters at this scale: the pixel rule merges almost everything
    assert not torch.equal(got, _batched(scores, boxes, [65, 40], 0.2, 0.45, **dict(kw, normalized=False)))


def test_special_columns():
    """No candidate; identical boxes; a suppression chain; a NaN score."""
    scores, boxes = dc.int_inputs([70], 5, 5, seed=14)
    scores[:, 1] = 0.0                                           # column 1: nothing passes
    boxes[:, 2] = torch.tensor([3.0, 4.0, 40.0, 30.0])           # column 2: identical boxes
    scores[:, 2] = 0.5                                           # ... and three rows sharing the top score
    scores[[11, 30, 42], 2] = 0.875
    scores[:, 3] = 0.0                                           # column 3: A kills B, B would kill C, C survives
    boxes[5, 3] = torch.tensor([10.0, 0.0, 29.0, 19.0])          # C
    boxes[9, 3] = torch.tensor([5.0, 0.0, 24.0, 19.0])           # B
    boxes[20, 3] = torch.tensor([0.0, 0.0, 19.0, 19.0])          # A
    scores[20, 3], scores[9, 3], scores[5, 3] = 0.875, 0.75, 0.5
    got = _batched(scores, boxes, [70], 0.25, dc.NMS_THRESH, skip_class=0)
    assert torch.equal(got, dc.oracle_mask(scores, boxes, [70], 8, 0))
    assert not got[:, 0].any() and not got[:, 1].any()
    top = torch.nonzero(scores[:, 2] == scores[:, 2].max()).reshape(-1)
    assert top.tolist() == [11, 30, 42] and torch.nonzero(got[:, 2]).reshape(-1).tolist() == [11]
    assert torch.nonzero(got[:, 3]).reshape(-1).tolist() == [5, 20]
    nan = scores.clone()
    nan[7, 4] = float("nan")
    low = scores.clone()
    low[7, 4] = 0.0
    for inclusive in (False, True):
        a = _batched(nan, boxes, [70], 0.25, dc.NMS_THRESH, skip_class=0, inclusive=inclusive)
        assert not a[7, 4] and torch.equal(a, _batched(low, boxes, [70], 0.25, dc.NMS_THRESH, skip_class=0,
                                                       inclusive=inclusive))


def test_every_keep_byte_is_rewritten():
    counts = [0, 65, 7]
    scores, boxes = dc.int_inputs(counts, 3, 3, seed=15)
    keep = torch.full((72, 3), 0xFF, dtype=torch.uint8, device="cuda")
    ov = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    D.nms_classes_launch(scores.cuda(), boxes.cuda(), [0, 0, 65, 72], 0.25, dc.NMS_THRESH, 0, False, -1, False, keep, ov)
    assert int(ov.item()) == 0 and int(keep.max()) == 1
    assert torch.equal(keep.cpu() == 1, dc.oracle_mask(scores, boxes, counts, 8, 0))


# --------------------------------------------------------------------------------------------- overflow
def test_overflow_falls_back_to_the_loop():
    cap = D.NMS_CLASSES_MIN_CAP
    scores, boxes = dc.int_inputs([5, cap + 1], 2, 2, seed=16)
    scores[5:, 0] = scores[5:, 0].clamp(min=0.5)                 # cap + 1 candidates in segment (1, 0)
    scores[5, 1] = 0.0                                           # and cap at most in the others
    got = D.multiclass_nms(scores.cuda(), boxes.cuda(), [5, cap + 1], 0.25, dc.NMS_THRESH, skip_class=-1, cap=cap)
    assert D.last_route("multiclass_nms") == "overflow"
    assert torch.equal(got.cpu(), _loop(scores, boxes, [5, cap + 1], 0.25, dc.NMS_THRESH, skip_class=-1))
    assert torch.equal(got.cpu(), dc.oracle_mask(scores, boxes, [5, cap + 1], 8, -1))
    # exactly cap candidates fit
    scores[5, 0] = 0.0
    got = _batched(scores, boxes, [5, cap + 1], 0.25, dc.NMS_THRESH, skip_class=-1, cap=cap)
    assert torch.equal(got, dc.oracle_mask(scores, boxes, [5, cap + 1], 8, -1))


# -------------------------------------------------------------------------------------- roi_align_levels
def _pyramid():
    g = torch.Generator().manual_seed(21)
    return [torch.randn(2, 5, 12, 16, generator=g).cuda(), torch.randn(2, 5, 6, 8, generator=g).cuda(),
            torch.randn(2, 5, 3, 4, generator=g).cuda()]


_SCALES = [0.25, 0.125, 0.0625]
_ROIS = torch.tensor([[0, 2.0, 3.0, 30.0, 20.0], [1, 0.0, 0.0, 60.0, 44.0], [1, 5.0, 5.0, 9.0, 9.0],
                      [0, -20.0, -8.0, 25.0, 30.0], [1, 40.0, 30.0, 90.0, 70.0], [0, 10.0, 4.0, 63.0, 47.0],
                      [1, 1.5, 2.5, 17.25, 40.0]])


def _levels_both(fmaps, rois, lv, sampling):
    got = D.roi_align_levels(fmaps, rois, lv, _SCALES, sampling, 7)
    assert D.last_route("roi_align_levels") == "batched"
    D.set_batched(False)
    ref = D.roi_align_levels(fmaps, rois, lv, _SCALES, sampling, 7)
    assert D.last_route("roi_align_levels") == "loop"
    D.set_batched(None)
    assert tuple(got.shape) == (rois.shape[0], 5, 7, 7) and torch.equal(got, ref)
    return got


@pytest.mark.parametrize("sampling", [0, 2])
@pytest.mark.parametrize("levels", [[0, 1, 2, 0, 2, 1, 0], [1] * 7, [0, 2, 0, 2, 2, 0, 0]],
                         ids=["mixed", "one-level", "level-without-roi"])
def test_roi_align_levels_bit_equal(levels, sampling):
    fmaps = _pyramid()
    rois = _ROIS.cuda()                                            # row 3 lies partly outside the map
    got = _levels_both(fmaps, rois, torch.tensor(levels, dtype=torch.int32).cuda(), sampling)
    for l in set(levels):                                          # and against the single-map kernel directly
        idx = torch.tensor([i for i, v in enumerate(levels) if v == l]).cuda()
        assert torch.equal(got[idx], D.roi_align(fmaps[l], rois[idx], _SCALES[l], sampling, 7, 7))
    assert bool(got.abs().sum() > 0)


def test_roi_align_levels_edges():
    fmaps = _pyramid()
    only1 = _ROIS[_ROIS[:, 0] == 1].cuda()                         # image 0 has no roi
    _levels_both(fmaps, only1, torch.tensor([1, 0, 2, 1], dtype=torch.int32).cuda(), 2)
    # levels outside [0, L-1] are clamped to the first / last map
    rois = _ROIS.cuda()
    out = _levels_both(fmaps, rois, torch.tensor([-1, 3, 0, 2, -1, 3, 1], dtype=torch.int32).cuda(), 2)
    ok = D.roi_align_levels(fmaps, rois, torch.tensor([0, 2, 0, 2, 0, 2, 1], dtype=torch.int32).cuda(), _SCALES, 2, 7)
    assert torch.equal(out, ok)
    empty = D.roi_align_levels(fmaps, rois[:0], torch.zeros(0, dtype=torch.int32).cuda(), _SCALES, 2, 7)
    assert tuple(empty.shape) == (0, 5, 7, 7)


def test_pooler_fixture_gpu():
    d = json.load(open(os.path.join(FIX, "pooler.json")))
    feats = T(torch.tensor(d["feature1"]).reshape(1, 2, 8, 8).cuda(), torch.tensor(d["feature2"]).reshape(1, 2, 4, 4).cuda(),
              torch.tensor(d["feature3"]).reshape(1, 2, 2, 2).cuda())
    rois = torch.tensor([[0, 0, 10, 10], [0, 0, 60, 60], [0, 0, 500, 500]], dtype=torch.float32).cuda()
    m = nn.Pooler(2, [0.125, 0.0625, 0.03125], 2)
    out = m.forward(T(feats, T(rois)))
    assert D.last_route("roi_align_levels") == "batched"
    assert torch.allclose(out.cpu().reshape(-1), torch.tensor(d["expectedRes"]), atol=1e-4)
    D.set_batched(False)
    assert torch.equal(m.forward(T(feats, T(rois))), out)


def test_pooler_two_images_batched_equals_loop():
    fmaps = _pyramid()
    rois = T(_ROIS[_ROIS[:, 0] == 0][:, 1:].cuda() * 4, torch.zeros(0, 4).cuda())   # scaled up: spans the levels
    m = nn.Pooler(7, _SCALES, 2)
    out = m.forward(T(T(*fmaps), rois))
    assert D.last_route("roi_align_levels") == "batched" and tuple(out.shape) == (3, 5, 7, 7)
    D.set_batched(False)
    assert torch.equal(m.forward(T(T(*fmaps), rois)), out)


# ---------------------------------------------------------------------------------------------- modules
def _module_both(run, monkeypatch):
    """Outputs with batching on — where the per-class loop must not run at all — equal the loop's."""
    def no_loop(*a, **kw):
        raise AssertionError("the per-class NMS loop ran on the batched path")

    with monkeypatch.context() as mp:
        mp.setattr(D, "nms_sorted", no_loop)
        D._ROUTE["multiclass_nms"] = None
        got = [t.clone() for t in dc.table_tensors(run())]
        assert D.last_route("multiclass_nms") == "batched"
    D.set_batched(False)
    ref = dc.table_tensors(run())
    D.set_batched(None)
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    return got


def test_box_post_processor_gpu(monkeypatch):
    logits, deltas, props, info = dc.box_post_inputs([70, 33], 6, seed=1, tie=True)
    props = T(props[1].cuda(), props[2].cuda())
    m = nn.BoxPostProcessor(0.05, 0.5, 5, 6).evaluate()
    out = _module_both(lambda: m.forward(T(logits.cuda(), deltas.cuda(), props, info.cuda())), monkeypatch)
    assert out[0].numel() > 10                                  # 2 images x maxPerImage 5, and the tie exceeds the cut
    m100 = nn.BoxPostProcessor(0.05, 0.5, 100, 6).evaluate()
    _module_both(lambda: m100.forward(T(logits.cuda(), deltas.cuda(), props, info.cuda())), monkeypatch)


def test_box_head_fixture_gpu(monkeypatch):
    d = json.load(open(os.path.join(FIX, "boxhead.json")))
    layer = nn.BoxHead(6, 7, [0.25, 0.125], 2, 0.012, 0.5, 100, 1024, 81)
    w, _ = layer.getParameters()
    w.fill_(0.001)
    layer.evaluate()
    layer.cuda()
    f1 = torch.tensor(d["features1"], dtype=torch.float32).cuda()
    f2 = torch.tensor(d["features2"], dtype=torch.float32).cuda()
    inp = T(T(f1, f2), T(torch.tensor(d["bbox"]).cuda()), torch.tensor(d["imageInfo"], dtype=torch.float32).cuda())
    with monkeypatch.context() as mp:
        mp.setattr(D, "nms_sorted", lambda *a, **kw: pytest.fail("the per-class NMS loop ran"))
        res = layer.forward(inp)[2]
    assert D.last_route("multiclass_nms") == "batched" and D.last_route("roi_align_levels") == "batched"
    assert res[1].tolist() == [float(c) for c in range(1, 81) for _ in range(2)]
    assert torch.allclose(res[2][1].cpu(), torch.tensor(d["expectedBbox"]), atol=1e-3)


def test_detection_output_frcnn_gpu(monkeypatch):
    fr = nn.DetectionOutputFrcnn(nClasses=3, maxPerImage=4).evaluate()
    rois = torch.tensor([[0, 10, 10, 50, 50], [0, 12, 12, 52, 52], [0, 100, 100, 150, 140]], dtype=torch.float32)
    scores = torch.tensor([[0.1, 0.8, 0.1], [0.1, 0.7, 0.2], [0.2, 0.1, 0.7]])
    info = torch.tensor([[200.0, 200.0, 1.0, 1.0]])
    o = _module_both(lambda: fr.forward(T(info.cuda(), rois.cuda(), torch.zeros(3, 12).cuda(), scores.cuda())),
                     monkeypatch)[0]
    assert int(o[0, 0]) == 4 and o[0, 1:].reshape(4, 6)[:, 0].tolist() == [1.0, 1.0, 2.0, 2.0]
    info, rois, deltas, scores = dc.frcnn_inputs(90, 4, seed=5)
    m = nn.DetectionOutputFrcnn(nClasses=4, maxPerImage=12).evaluate()
    o = _module_both(lambda: m.forward(T(info.cuda(), rois.cuda(), deltas.cuda(), scores.cuda())), monkeypatch)[0]
    assert int(o[0, 0]) == 12


@pytest.mark.parametrize("share", [True, False])
def test_detection_output_ssd_gpu(monkeypatch, share):
    loc, conf, prior = dc.ssd_inputs(2, 4, share, seed=7)
    m = nn.DetectionOutputSSD(nClasses=4, keepTopK=5, shareLocation=share).evaluate()
    o = _module_both(lambda: m.forward(T(loc.cuda(), conf.cuda(), prior.cuda())), monkeypatch)[0]
    assert tuple(o.shape) == (2, 31) and int(o[0, 0]) == 5
    all_ = nn.DetectionOutputSSD(nClasses=4, keepTopK=-1, nmsTopk=6, shareLocation=share).evaluate()
    _module_both(lambda: all_.forward(T(loc.cuda(), conf.cuda(), prior.cuda())), monkeypatch)


# ------------------------------------------------------------------------------------------- HIP graph
def test_launch_replays_from_a_hip_graph():
    counts = [0, 65, 7]
    off = [0, 0, 65, 72]
    s0, b0 = dc.float_inputs(counts, 3, 3, seed=31)
    s1, b1 = dc.float_inputs(counts, 3, 3, seed=32)
    scores, boxes = s0.cuda(), b0.cuda()
    keep = torch.empty(72, 3, dtype=torch.uint8, device="cuda")
    ov = torch.empty(1, dtype=torch.int32, device="cuda")

    def launch():
        D.nms_classes_launch(scores, boxes, off, 0.3, 0.45, 0, False, -1, False, keep, ov)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    first = keep.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    scores.copy_(s1)
    boxes.copy_(b1)
    keep.fill_(0xFF)
    ov.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    assert int(ov.item()) == 0
    assert torch.equal(keep.bool(), D.multiclass_nms(s1.cuda(), b1.cuda(), counts, 0.3, 0.45))
    assert torch.equal(first.bool(), D.multiclass_nms(s0.cuda(), b0.cuda(), counts, 0.3, 0.45))
    assert not torch.equal(first, keep)
