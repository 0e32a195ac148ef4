"""segmented_topk_*_kernel (csrc/detection.hip), ops.detection.rpn_select and RegionProposal on the GPU: top-k
indices against the pure-Python oracle and torch.sort(stable=True), the gathered rows against indexing, rpn_select
batched against its loop form, its NMS stage against the integer oracle, and the module batched against the
per-image loop module and against rpn_select's loop form on the real head's outputs (GPU only)."""
import pytest
import torch

from bigdl_amd import nn
from bigdl_amd.ops import detection as D
from bigdl_amd.utils.table import T, Table
from tests import detection_batched_cases as dc
from tests import rpn_batched_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_switch():
    D.set_batched(None)
    yield
    D.set_batched(None)


_FLAT = {}


def _flat_case(kind):
    """(values, offsets) of one flat call, built once per kind."""
    if kind not in _FLAT:
        off = rc.offsets(rc.FLAT_LENGTHS)
        make = {"uniform": rc.uniform_values, "quantised": rc.quantised_values, "special": rc.special_values}[kind]
        _FLAT[kind] = (make(off[-1], seed=7), off)
    return _FLAT[kind]


# ------------------------------------------------------------------------------------------- flat mode
def test_special_values_sort_as_torch_sorts_them():
    v = torch.tensor(rc.SPECIAL)
    got = D.segmented_topk(v.cuda(), [0, len(rc.SPECIAL)], len(rc.SPECIAL))
    assert got.indices.cpu().tolist() == rc.SPECIAL_ORDER
    assert got.indices.cpu().tolist() == torch.sort(v, descending=True, stable=True).indices.tolist()
    assert torch.equal(got.values.cpu().view(torch.int32), v[rc.SPECIAL_ORDER].view(torch.int32))


@pytest.mark.parametrize("k", rc.KS)
@pytest.mark.parametrize("kind", ["uniform", "quantised", "special"])
def test_flat_topk_against_oracle_and_stable_sort(kind, k):
    values, off = _flat_case(kind)
    got = D.segmented_topk(values.cuda(), off, k)
    assert got.counts is None and got.indices.dtype == torch.int32
    rc.check_flat(got, values, off, k)
    idx = got.indices.cpu()
    for s, n in enumerate(rc.FLAT_LENGTHS):
        order = torch.sort(values[off[s]:off[s + 1]], descending=True, stable=True).indices[:k]
        assert torch.equal(idx[got.offsets[s]:got.offsets[s + 1]].long(), order)
    if kind == "quantised":                                   # a run of ties straddles the cut of the long segment
        seg = values[off[-2]:]
        ranked = seg[torch.sort(seg, descending=True, stable=True).indices]
        assert ranked[k - 1] == ranked[k]


@pytest.mark.parametrize("k", rc.KS)
def test_flat_topk_all_equal_segment(k):
    lengths = [3, 5000, 70]
    off = rc.offsets(lengths)
    values = rc.uniform_values(off[-1], seed=k)
    values[off[1]:off[2]] = 0.375
    rc.check_flat(D.segmented_topk(values.cuda(), off, k), values, off, k)


@pytest.mark.parametrize("k", rc.KS)
@pytest.mark.parametrize("kind", ["quantised", "special"])
def test_flat_topk_with_mask(kind, k):
    values, off = _flat_case(kind)
    g = torch.Generator().manual_seed(k)
    mask = (torch.rand(off[-1], generator=g) < 0.5).to(torch.uint8)
    mask[off[5]:off[6]] = 0                                   # 1023 elements: the mask removes everything
    mask[off[8]:off[9]] = 0                                   # 8193 elements: the mask leaves 40, fewer than most k
    mask[off[8]:off[9]][torch.randperm(8193, generator=g)[:40]] = 1
    got = D.segmented_topk(values.cuda(), off, k, mask=mask.cuda())
    rc.check_flat(got, values, off, k, mask)
    counts = got.counts.cpu().tolist()
    assert counts[0] == 0 and counts[5] == 0 and counts[8] == min(k, 40)
    assert counts[9] == min(k, int(mask[off[9]:].sum()))
    both = D.segmented_topk(values.cuda(), off, k, mask=mask.bool().cuda(), global_index=True)
    for s in range(len(rc.FLAT_LENGTHS)):
        a = got.indices[got.offsets[s]:got.offsets[s] + counts[s]] + off[s]
        assert torch.equal(both.indices[got.offsets[s]:got.offsets[s] + counts[s]], a)


def test_flat_topk_more_segments_than_one_launch_holds():
    lengths = [(7 * s) % 23 for s in range(150)]
    off = rc.offsets(lengths)
    values = rc.quantised_values(off[-1], seed=2)
    rc.check_flat(D.segmented_topk(values.cuda(), off, 5), values, off, 5)


# -------------------------------------------------------------------------------------- level-map mode
MAP_SHAPES = [(7, 5), (13, 9), (120, 200)]


@pytest.mark.parametrize("N,k,kind", [(1, 50, "uniform"), (1, 4096, "quantised"), (3, 50, "quantised"),
                                      (3, 4096, "uniform"), (3, 1000, "special")])
def test_level_maps_against_oracle_and_indexing(N, k, kind):
    A = 3
    make = {"uniform": rc.uniform_values, "quantised": rc.quantised_values, "special": rc.special_values}[kind]
    g = torch.Generator().manual_seed(N * 10000 + k)
    obj = [make(N * A * h * w, seed=N + k + h).reshape(N, A, h, w) for h, w in MAP_SHAPES]
    reg = [torch.randn(N, 4 * A, h, w, generator=g) for h, w in MAP_SHAPES]
    anc = [torch.randn(h * w * A, 4, generator=g) for h, w in MAP_SHAPES]
    got = D.segmented_topk([o.cuda() for o in obj], k=k, regression=[r.cuda() for r in reg],
                           anchors=[a.cuda() for a in anc])
    idx, val = got.indices.cpu().long(), got.values.cpu()
    greg, ganc = got.regression.cpu(), got.anchors.cpu()
    assert len(got.offsets) == N * len(MAP_SHAPES) + 1 and got.counts is None
    for n in range(N):
        for l, (h, w) in enumerate(MAP_SHAPES):
            s = n * len(MAP_SHAPES) + l
            lo, hi = got.offsets[s], got.offsets[s + 1]
            assert hi - lo == min(k, h * w * A)
            flat = obj[l][n].permute(1, 2, 0).reshape(-1)
            rows = reg[l][n].reshape(A, 4, h, w).permute(2, 3, 0, 1).reshape(-1, 4)
            order = torch.sort(flat, descending=True, stable=True).indices[:k]
            assert torch.equal(idx[lo:hi], order), f"image {n} level {l}"
            if h * w * A <= 8192 or n == 0:                   # the Python oracle on the long level once per case
                assert idx[lo:hi].tolist() == rc.oracle_topk(flat.tolist(), k)
            assert torch.equal(val[lo:hi].view(torch.int32), flat[order].view(torch.int32))
            assert torch.equal(greg[lo:hi], rows[order])
            assert torch.equal(ganc[lo:hi], anc[l][order])


# -------------------------------------------------------------------------------------------- rpn_select
def _both_forms(obj, reg, anc, size, pre, post, thresh):
    args = ([o.cuda() for o in obj], [r.cuda() for r in reg], [a.cuda() for a in anc], size, pre, post, thresh)
    got = D.rpn_select(*args)
    assert D.last_route("rpn_select") == "batched" and D.last_route() == "batched"
    D.set_batched(False)
    try:
        ref = D.rpn_select(*args)
        assert D.last_route("rpn_select") == "loop"
    finally:
        D.set_batched(None)
    assert len(got) == len(ref) == obj[0].shape[0]
    for g, r in zip(got, ref):
        assert g.shape == r.shape and torch.equal(g, r)
    return [g.cpu() for g in got]


@pytest.mark.parametrize("N", [1, 2, 3])
def test_rpn_select_batched_equals_loop(N):
    shapes, size = [(16, 16), (8, 8), (4, 4)], (64.0, 64.0)
    obj, reg = rc.rpn_inputs(N, shapes, 3, seed=20 + N)
    anc = rc.anchors_for([32, 64, 128], [0.5, 1, 2], [4, 8, 16], shapes)
    got = _both_forms(obj, reg, anc, size, 50, 20, 0.7)
    # not vacuous (figures of the CPU pipeline): a level shorter than pre_topk, NMS removes and keeps, the cut cuts
    _, stages = rc.oracle_rpn(obj, reg, anc, size, 50, 20, 0.7)
    assert any(c < 50 for c, _ in stages) and all(k > 0 for _, k in stages) and any(k < c for c, k in stages)
    for b in range(N):
        assert sum(k for _, k in stages[3 * b:3 * b + 3]) > 20 == got[b].shape[0]


def test_rpn_select_batched_equals_loop_k_1000_on_a_long_level():
    shapes, size = [(40, 64), (20, 32)], torch.tensor([160.0, 256.0])
    obj, reg = rc.rpn_inputs(2, shapes, 3, seed=31)
    obj[0] = (obj[0] * 4).round() / 4                          # ties on the 7680-element level
    anc = rc.anchors_for([32, 64], [0.5, 1, 2], [4, 8], shapes)
    got = _both_forms(obj, reg, anc, size, 1000, 300, 0.7)
    assert all(g.shape == (300, 4) for g in got)
    dev = _both_forms(obj, reg, anc, size.cuda(), 1000, 300, 0.7)   # a device image size is not read back
    assert all(torch.equal(a, b) for a, b in zip(got, dev))


def test_rpn_select_nan_and_inf_logits():
    shapes, size = [(8, 8), (4, 4)], (64.0, 64.0)
    obj, reg = rc.rpn_inputs(2, shapes, 3, seed=5)
    obj = [(o * 2).round() / 2 for o in obj]
    obj[0][0, 1, 2, 3] = float("nan")
    obj[1][1, 0, 0, 0] = float("inf")
    anc = rc.anchors_for([32, 64], [0.5, 1, 2], [8, 16], shapes)
    _both_forms(obj, reg, anc, size, 30, 10, 0.7)


def test_rpn_select_outside_the_limits_takes_the_loop():
    shapes = [(4, 4)]
    obj, reg = rc.rpn_inputs(1, shapes, 3, seed=1)
    anc = rc.anchors_for([32], [0.5, 1, 2], [16], shapes)
    D.rpn_select([obj[0].cuda()], [reg[0].cuda()], [anc[0].cuda()], (64.0, 64.0), 5000, 20, 0.7)
    assert D.last_route("rpn_select") == "loop"


@pytest.mark.parametrize("counts", [[5, 64, 65, 0, 300], [1030, 257], [4096]])
def test_nms_stage_equals_integer_oracle(counts):
    _, boxes = dc.int_inputs(counts, 1, 1, seed=sum(counts))
    off = rc.offsets(counts)
    keep = D.rpn_nms_launch(boxes.reshape(-1, 4).cuda(), off, dc.NMS_THRESH).cpu()
    bi = boxes.reshape(-1, 4).long().tolist()
    want = torch.zeros(off[-1], dtype=torch.uint8)
    for s, n in enumerate(counts):                            # rank order is row order: score = a descending ramp
        for r in dc.oracle_segment([n - r for r in range(n)], bi[off[s]:off[s + 1]], -1):
            want[off[s] + r] = 1
    assert torch.equal(keep, want)
    assert 0 < int(want.sum()) < off[-1]


# ------------------------------------------------------------------------------------------------ module
def _forward(rp, feats, size, batched):
    D.set_batched(batched)
    try:
        return [t.clone() for t in dc.table_tensors(rp.forward(T(feats, size)))]
    finally:
        D.set_batched(None)


@pytest.mark.parametrize("N", [1, 2])
def test_module_batched_equals_loop_module(N):
    rp, feats, size = rc.module_case(N, seed=N)
    for b in range(N):                                        # precondition: torch.topk has no tie to break
        sg = torch.sigmoid(rc.module_logits(feats, b).cuda())
        assert torch.unique(sg).numel() == sg.numel()
    dev = Table()
    for i in range(feats.length()):
        dev[i + 1] = feats[i + 1].cuda()
    D._set_route("rpn_select", None)
    ref = _forward(rp, dev, size, False)
    assert D.last_route("rpn_select") is None                 # the per-image loop module does not call the op
    got = _forward(rp, dev, size, True)
    assert D.last_route("rpn_select") == "batched"
    assert len(got) == len(ref) == N
    for g, r in zip(got, ref):
        assert g.shape == (20, 4) and torch.equal(g, r)
    again = _forward(rp, dev, size, True)                     # cached anchors
    assert all(torch.equal(a, g) for a, g in zip(again, got))


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("train", [False, True])
def test_module_with_the_conv_head_equals_loop_form_on_its_outputs(N, train):
    torch.manual_seed(3)
    rp = nn.RegionProposal(16, [32, 64, 128], [0.5, 1, 2], [4, 8, 16], 50, 20, 80, 30).to("cuda")
    rp = rp.training() if train else rp.evaluate()
    g = torch.Generator().manual_seed(N)
    shapes = rc.MODULE_SHAPES
    feats = Table()
    for i, (h, w) in enumerate(shapes):
        feats[i + 1] = (torch.randn(N, 16, h, w, generator=g) * 20).cuda()
    size = torch.tensor([64.0, 64.0])
    got = _forward(rp, feats, size, True)
    assert D.last_route("rpn_select") == "batched"
    obj, reg = [], []
    for i in range(len(shapes)):
        ho = rp.head.forward(feats[i + 1])
        obj.append(ho[1].clone())
        reg.append(ho[2].clone())
    anc = [a.cuda() for a in rc.anchors_for([32, 64, 128], [0.5, 1, 2], [4, 8, 16], shapes)]
    D.set_batched(False)
    ref = D.rpn_select(obj, reg, anc, size, 80 if train else 50, 30 if train else 20, 0.7)
    assert D.last_route("rpn_select") == "loop"
    assert len(got) == len(ref) == N
    for a, b in zip(got, ref):
        assert torch.equal(a, b) and 0 < a.shape[0] <= (30 if train else 20)
