"""multiclass_nms / roi_align_levels and the modules built on them, on the CPU engine: the op's loop path against
a pure-integer greedy-NMS oracle and against the modules' per-class loop, and the switch in its three forms."""
import pytest
import torch

from bigdl_amd import nn
from bigdl_amd.nn import detection as ND
from bigdl_amd.ops import detection as D
from bigdl_amd.utils.table import T
from tests import detection_batched_cases as dc


@pytest.fixture(autouse=True)
def _default_switch():
    yield
    D.set_batched(None)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129, 300])
def test_nms_agrees_with_integer_oracle(n):
    scores, boxes = dc.int_inputs([n], 1, 1, seed=n)
    kept = dc.oracle_segment((scores[:, 0] * 32).long().tolist(), boxes[:, 0].long().tolist(), -1)
    got = D.nms(scores[:, 0], boxes[:, 0], dc.NMS_THRESH)
    assert set(got.tolist()) == kept
    if n >= 63:                                   # the yardstick both suppresses and keeps a real share of the boxes
        assert 0.1 * n <= n - len(kept) <= 0.6 * n


@pytest.mark.parametrize("counts,C,Cb,skip,inclusive,topk", [
    ([65], 3, 3, 0, False, -1), ([0, 65, 7], 3, 3, -1, False, -1), ([129], 3, 1, 0, True, -1),
    ([300], 2, 2, -1, True, 10), ([1], 3, 3, 0, False, 500)])
def test_multiclass_nms_cpu_equals_oracle(counts, C, Cb, skip, inclusive, topk):
    scores, boxes = dc.int_inputs(counts, C, Cb, seed=sum(counts) + C)
    got = D.multiclass_nms(scores, boxes, counts, 0.25, dc.NMS_THRESH, skip_class=skip, inclusive=inclusive,
                           pre_topk=topk)
    assert D.last_route("multiclass_nms") == "loop" and D.last_route() == "loop"
    assert got.dtype == torch.bool and tuple(got.shape) == tuple(scores.shape)
    assert torch.equal(got, dc.oracle_mask(scores, boxes, counts, 8, skip, inclusive, topk))


def test_multiclass_nms_equals_per_class_nms():
    scores, boxes = dc.float_inputs([90], 5, 5, seed=4)
    got = D.multiclass_nms(scores, boxes, [90], 0.3, 0.4)
    res = ND._per_class_nms(scores, boxes.reshape(90, 20), 5, 0.3, 0.4, True)
    assert not got[:, 0].any()
    for c in range(1, 5):
        rows = torch.nonzero(got[:, c]).reshape(-1)
        assert torch.equal(scores[rows, c], res[c][0]) and torch.equal(boxes[rows, c], res[c][1])


def test_roi_align_levels_cpu_equals_per_level():
    g = torch.Generator().manual_seed(2)
    fmaps = [torch.randn(2, 3, 12, 16, generator=g), torch.randn(2, 3, 6, 8, generator=g)]
    rois = torch.tensor([[0, 2.0, 3.0, 30.0, 20.0], [1, 0.0, 0.0, 60.0, 44.0], [1, 5.0, 5.0, 9.0, 9.0]])
    lv = torch.tensor([0, 1, 0], dtype=torch.int32)
    out = D.roi_align_levels(fmaps, rois, lv, [0.25, 0.125], 2, 7)
    assert D.last_route("roi_align_levels") == "loop"
    assert torch.equal(out[1], D.roi_align(fmaps[1], rois[1:2], 0.125, 2, 7, 7)[0])
    assert torch.equal(out[[0, 2]], D.roi_align(fmaps[0], rois[[0, 2]], 0.25, 2, 7, 7))


def test_switch_three_forms(monkeypatch):
    from bigdl_amd.utils.engine import Engine

    assert D.batched(True) and not D.batched(False)          # default: on where the kernels run
    monkeypatch.setenv("BIGDL_DET_BATCHED", "0")
    assert not D.batched(True)
    D.set_batched(True)
    assert D.batched(True) and not D.batched(False)          # the CPU engine keeps the loop
    Engine.setProperty("bigdl.detection.batched", "false")
    assert not D.batched(True)
    D.set_batched(None)
    monkeypatch.delenv("BIGDL_DET_BATCHED")
    assert D.batched(True)


class _MaskPath:
    """ops.detection as the modules see it, with ``batched`` always on: the modules then select their outputs from
    the multiclass_nms / roi_align_levels results, which the ops build from their loops on CPU tensors."""
    batched = staticmethod(lambda is_cuda: True)

    def __getattr__(self, name):
        return getattr(D, name)


def _both(run, monkeypatch):
    outs = []
    for on in (True, False):
        D.set_batched(on)
        outs.append([t.clone() for t in dc.table_tensors(run())])
    assert len(outs[0]) == len(outs[1]) and all(torch.equal(a, b) for a, b in zip(*outs))
    monkeypatch.setattr(ND, "D", _MaskPath())
    D._ROUTE.update({"multiclass_nms": None, "roi_align_levels": None})
    mask = dc.table_tensors(run())
    assert "loop" in (D.last_route("multiclass_nms"), D.last_route("roi_align_levels"))   # the ops were called
    assert len(mask) == len(outs[0]) and all(torch.equal(a, b) for a, b in zip(mask, outs[0]))
    return outs[0]


def test_box_post_processor_switch_cpu(monkeypatch):
    logits, deltas, props, info = dc.box_post_inputs([70, 33], 6, seed=1, tie=True)
    m = nn.BoxPostProcessor(0.05, 0.5, 5, 6).evaluate()
    out = _both(lambda: m.forward(T(logits, deltas, props, info)), monkeypatch)
    assert out[0].numel() >= 10


def test_detection_output_frcnn_switch_cpu(monkeypatch):
    info, rois, deltas, scores = dc.frcnn_inputs(90, 4, seed=5)
    m = nn.DetectionOutputFrcnn(nClasses=4, maxPerImage=12).evaluate()
    out = _both(lambda: m.forward(T(info, rois, deltas, scores)), monkeypatch)
    assert int(out[0][0, 0]) == 12


@pytest.mark.parametrize("share", [True, False])
def test_detection_output_ssd_switch_cpu(monkeypatch, share):
    loc, conf, prior = dc.ssd_inputs(2, 4, share, seed=7)
    m = nn.DetectionOutputSSD(nClasses=4, keepTopK=5, shareLocation=share).evaluate()
    out = _both(lambda: m.forward(T(loc, conf, prior)), monkeypatch)
    assert int(out[0][0, 0]) == 5


def test_pooler_switch_cpu(monkeypatch):
    g = torch.Generator().manual_seed(3)
    feats = T(torch.randn(2, 5, 12, 16, generator=g), torch.randn(2, 5, 6, 8, generator=g))
    rois = T(torch.tensor([[1.0, 3.0, 20.0, 26.0], [0.0, 0.0, 400.0, 300.0]]), torch.tensor([[3.0, 5.0, 36.0, 27.0]]))
    m = nn.Pooler(7, [0.25, 0.125], 2)
    out = _both(lambda: m.forward(T(feats, rois)), monkeypatch)
    assert tuple(out[0].shape) == (3, 5, 7, 7)
