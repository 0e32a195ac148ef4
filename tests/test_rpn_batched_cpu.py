"""The loop forms of ops.detection.segmented_topk / rpn_select on the CPU against the pure-Python oracles of
rpn_batched_cases, and RegionProposal on CPU tensors, which keeps its per-image loop whatever the batching switch
says."""
import pytest
import torch

from bigdl_amd.ops import detection as D
from tests import rpn_batched_cases as rc
from tests.detection_batched_cases import table_tensors


@pytest.fixture(autouse=True)
def _default_switch():
    D.set_batched(None)
    yield
    D.set_batched(None)


def test_oracle_gives_the_order_of_a_stable_descending_sort():
    v = torch.tensor(rc.SPECIAL)
    assert rc.oracle_topk(rc.SPECIAL, len(rc.SPECIAL)) == rc.SPECIAL_ORDER
    assert torch.sort(v, descending=True, stable=True).indices.tolist() == rc.SPECIAL_ORDER


@pytest.mark.parametrize("k", [1, 50, 4096])
@pytest.mark.parametrize("make", [rc.uniform_values, rc.quantised_values, rc.special_values])
def test_flat_topk_loop_against_oracle(make, k):
    lengths = [0, 1, 9, 255, 257, 1025]
    off = rc.offsets(lengths)
    values = make(off[-1], seed=k)
    rc.check_flat(D.segmented_topk(values, off, k), values, off, k)
    mask = (torch.rand(off[-1], generator=torch.Generator().manual_seed(k + 1)) < 0.3).to(torch.uint8)
    mask[off[3]:off[4]] = 0                                   # one segment loses everything
    got = D.segmented_topk(values, off, k, mask=mask)
    rc.check_flat(got, values, off, k, mask)
    assert got.counts[3] == 0


def test_flat_topk_loop_global_index():
    off = rc.offsets([5, 0, 7])
    values = rc.quantised_values(12, seed=3)
    local = D.segmented_topk(values, off, 4)
    glob = D.segmented_topk(values, off, 4, global_index=True)
    assert glob.indices.tolist() == [i + off[s] for s in range(3)
                                     for i in local.indices[local.offsets[s]:local.offsets[s + 1]].tolist()]


@pytest.mark.parametrize("N", [1, 2])
def test_rpn_select_loop_against_oracle(N):
    shapes, size = [(16, 16), (8, 8), (4, 4)], (64.0, 64.0)
    obj, reg = rc.rpn_inputs(N, shapes, 3, seed=10 + N)
    anc = rc.anchors_for([32, 64, 128], [0.5, 1, 2], [4, 8, 16], shapes)
    D.set_batched(True)                                       # CPU tensors: still the loop
    got = D.rpn_select(obj, reg, anc, size, 50, 20, 0.7)
    assert D.last_route("rpn_select") == "loop"
    want, stages = rc.oracle_rpn(obj, reg, anc, size, 50, 20, 0.7)
    assert len(got) == N
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    # not vacuous: a level shorter than pre_topk, NMS both removes and keeps, the final cut is active
    assert any(c < 50 for c, _ in stages) and all(0 < k for _, k in stages) and any(k < c for c, k in stages)
    for b in range(N):
        assert sum(k for _, k in stages[3 * b:3 * b + 3]) > 20 == want[b].shape[0]


def test_rpn_select_loop_ties_and_nan_follow_the_defined_order():
    shapes, size = [(8, 8), (4, 4)], (64.0, 64.0)
    obj, reg = rc.rpn_inputs(2, shapes, 3, seed=5)
    obj = [(o * 2).round() / 2 for o in obj]                  # multiples of 1/2: ties at every cut
    obj[0][0, 1, 2, 3] = float("nan")
    obj[1][1, 0, 0, 0] = float("inf")
    anc = rc.anchors_for([32, 64], [0.5, 1, 2], [8, 16], shapes)
    got = D.rpn_select(obj, reg, anc, size, 30, 10, 0.7)
    want, _ = rc.oracle_rpn(obj, reg, anc, size, 30, 10, 0.7)
    for g, w in zip(got, want):
        assert torch.equal(g, w)


@pytest.mark.parametrize("N", [1, 2])
def test_module_on_cpu_keeps_its_loop(N):
    rp, feats, size = rc.module_case(N, seed=N)
    for b in range(N):                                        # precondition: torch.topk has no tie to break
        sg = torch.sigmoid(rc.module_logits(feats, b))
        assert torch.unique(sg).numel() == sg.numel()
    D._set_route("rpn_select", None)
    D.set_batched(False)
    ref = [t.clone() for t in table_tensors(rp.forward(D_table(feats, size)))]
    D.set_batched(True)
    got = table_tensors(rp.forward(D_table(feats, size)))
    assert D.last_route("rpn_select") is None                 # the module's own per-image loop ran both times
    assert len(got) == len(ref) == N
    for g, r in zip(got, ref):
        assert torch.equal(g, r) and g.shape == (20, 4)
    # the op's loop form on the same logits and regression gives the module's boxes
    obj = [feats[i + 1][:, :3] for i in range(3)]
    reg = [feats[i + 1][:, 3:15] for i in range(3)]
    anc = rc.anchors_for([32, 64, 128], [0.5, 1, 2], [4, 8, 16], rc.MODULE_SHAPES)
    sel = D.rpn_select(obj, reg, anc, size, 50, 20, 0.7)
    assert D.last_route("rpn_select") == "loop"
    for g, r in zip(sel, ref):
        assert torch.equal(g, r)


def D_table(feats, size):
    from bigdl_amd.utils.table import T

    return T(feats, size)
