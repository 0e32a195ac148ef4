"""BinaryTreeLSTM on the fused level kernels (csrc/treelstm.hip, ops/tree_lstm.py) against the module's CPU loop in
fp64: accuracy relative to the loop route's own error, exact indexing under renumbering, reproducibility, fallback."""
import copy
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

PAD = [-1, -1, -1]
BALANCED = [[2, 3, -1], [4, 5, 0], [6, 7, 0], [0, 0, 1], [0, 0, 2], [0, 0, 3], [0, 0, 4]]
SMALL = [[2, 5, -1], [0, 0, 1], [0, 0, 2], [0, 0, 3], [3, 4, 0]]
SAME_WORD = [[2, 3, -1], [4, 5, 0], [6, 7, 0], [0, 0, 1], [0, 0, 2], [0, 0, 2], [0, 0, 4]]      # word 3 is unused
SHARED = [[2, 3, -1], [4, 5, 0], [5, 6, 0], [0, 0, 1], [0, 0, 2], [0, 0, 3]]                    # node 5: two parents
ERRORS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                      "treelstm_fused_errors.txt")
_logged = []


def _chain(k):
    """Left-deep chain of k leaves: composers 1..k-1 (a level of one node each), leaves k..2k-1."""
    rows = [[i + 1 if i < k - 1 else 2 * k - 1, k + i - 1, -1 if i == 1 else 0] for i in range(1, k)]
    return rows + [[0, 0, j + 1] for j in range(k)]


def _batch(trees):
    n = max(len(t) for t in trees)
    return torch.tensor([t + [PAD] * (n - len(t)) for t in trees], dtype=torch.float32)


BATCHES = {
    "single_leaf": (_batch([[[0, 0, -1]], SMALL + [PAD]]), 3),
    "chains": (_batch([_chain(9), _chain(9) + [PAD]]), 9),
    "balanced20": (_batch([BALANCED] * 20), 4),
    "same_word": (_batch([SAME_WORD, BALANCED]), 4),
}


@pytest.fixture(autouse=True)
def _switch():
    from bigdl_amd.ops import tree_lstm

    yield
    tree_lstm.set_fused(None)


def _model(H, I, gate, seed=3):
    from bigdl_amd import nn
    from bigdl_amd.utils.random_generator import RNG

    RNG.setSeed(seed)
    return nn.BinaryTreeLSTM(I, H, gateOutput=gate)


def _run(m, x, trees, gy, fused=None):
    """[output, gradInput, six parameter gradients] of one forward + backward (``fused`` sets the switch)."""
    from bigdl_amd.ops import tree_lstm
    from bigdl_amd.utils.table import Table

    if fused is not None:
        tree_lstm.set_fused(fused)
    m.zeroGradParameters()
    inp = Table(x, trees)
    out = m.forward(inp).clone()
    gi = m.backward(inp, gy)
    assert not gi[2].any()                                   # the trees' gradInput is all zeros
    return [out, gi[1].clone()] + [g.clone() for g in m.parameters()[1]], tree_lstm.last_route()


def _fp64(m):
    ref = copy.deepcopy(m)
    for w, g in ref._params:
        setattr(ref, w, getattr(ref, w).double())
        setattr(ref, g, getattr(ref, g).double())
    return ref


def _err(a, ref):
    return float((a.double().cpu() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("name", list(BATCHES))
@pytest.mark.parametrize("H,I,gate", [(24, 20, True), (64, 64, False), (150, 20, True), (150, 64, False)])
def test_fused_matches_fp64_within_twice_the_loop_error(name, H, I, gate):
    """Every quantity of the fused route is within 2 x the loop route's own error against the fp64 CPU loop (+ 1e-6):
    both round the same operands to bf16 and accumulate in fp32, the factor covers the summation order."""
    trees, L = BATCHES[name]
    g = torch.Generator().manual_seed(11)
    x = torch.randn(trees.shape[0], L, I, generator=g)
    gy = torch.randn(trees.shape[0], trees.shape[1], H, generator=g)      # non-zero on padding rows too
    m = _model(H, I, gate)
    ref, _ = _run(_fp64(m), x.double(), trees, gy.double())
    gpu = copy.deepcopy(m).to("cuda")
    loop, route_l = _run(gpu, x.cuda(), trees.cuda(), gy.cuda(), fused=False)
    fused, route_f = _run(gpu, x.cuda(), trees.cuda(), gy.cuda(), fused=True)
    assert (route_l, route_f) == ("loop", "fused")
    names = ["output", "gradInput", "leafW", "leafB", "leftW", "leftB", "rightW", "rightB"]
    pairs = [(n, _err(f, r), _err(l, r)) for n, f, l, r in zip(names, fused, loop, ref)]
    os.makedirs(os.path.dirname(ERRORS), exist_ok=True)
    with open(ERRORS, "a" if _logged else "w") as f:
        _logged.append(1)
        for n, ef, el in pairs:
            f.write(f"{name} H={H} I={I} gateOutput={gate} {n}: fused {ef:.3e} loop {el:.3e}\n")
    for n, ef, el in pairs:
        assert ef <= 2 * el + 1e-6, (n, ef, el)


def _renumbered(trees, x, gy, g):
    """The same batch with the nodes of every tree renumbered (padding rows stay last) and the trees permuted:
    (trees, x, gy, index) with new[index[0], index[1]] = old for [B, N, .] tensors."""
    B, N = trees.shape[:2]
    bp = torch.randperm(B, generator=g)
    node = torch.arange(N).repeat(B, 1)
    new = trees.clone()
    for b in range(B):
        r = int((trees[b, :, 0] != -1).sum())
        node[b, :r] = torch.randperm(r, generator=g)
        kids = trees[b, :, :2].long()
        new[bp[b], node[b], :2] = torch.where(kids > 0, node[b][(kids - 1).clamp(min=0)] + 1, kids).float()
        new[bp[b], node[b], 2] = trees[b, :, 2]
    idx = (bp[:, None].expand(B, N), node)
    gy2 = torch.empty_like(gy)
    gy2[idx] = gy
    x2 = torch.empty_like(x)
    x2[bp] = x
    return new, x2, gy2, idx, bp


def test_fused_indexing_is_exact_and_reproducible():
    """Renumbering the nodes and permuting the batch moves the results and changes no bit; a second run of the same
    inputs is bitwise equal; padding rows, unreachable nodes and unused words get exactly 0."""
    trees = _batch([SAME_WORD + [[0, 0, 2], PAD], _chain(5), [[0, 0, -1]]])      # node 8 of tree 0 is unreachable
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 5, 20, generator=g)
    gy = torch.randn(3, 9, 150, generator=g)
    m = _model(150, 20, True).to("cuda")
    (out, gi, *_), route = _run(m, x.cuda(), trees.cuda(), gy.cuda(), fused=True)
    assert route == "fused"
    (out_b, gi_b, *_), _ = _run(m, x.cuda(), trees.cuda(), gy.cuda())
    assert torch.equal(out, out_b) and torch.equal(gi, gi_b)
    t2, x2, gy2, idx, bp = _renumbered(trees, x, gy, g)
    (out2, gi2, *_), route = _run(m, x2.cuda(), t2.cuda(), gy2.cuda())
    assert route == "fused"
    assert torch.equal(out2.cpu()[idx], out.cpu()) and torch.equal(gi2.cpu()[bp], gi.cpu())
    assert out.abs().sum() > 0 and not out[0, 7:].any() and not out[2, 1:].any()
    assert not gi[0, 2].any() and not gi[0, 4].any() and gi[0, 1].any()          # words 3 and 5 of tree 0 are unused
    assert gi[2, 3].any() and not gi[2, :3].any() and not gi[2, 4].any()         # a root leaf (tag -1) indexes word -2, as the loop does


def test_fallback_routes():
    """A tree that shares a child between two parents, the switch off and CPU tensors all run the loop."""
    trees, g = _batch([SHARED, SMALL + [PAD]]), torch.Generator().manual_seed(2)
    x, gy = torch.randn(2, 3, 20, generator=g), torch.randn(2, 6, 24, generator=g)
    cpu = _model(24, 20, True)
    m = copy.deepcopy(cpu).to("cuda")
    (out_off, *_), route_off = _run(m, x.cuda(), trees.cuda(), gy.cuda(), fused=False)
    (out_on, *_), route_on = _run(m, x.cuda(), trees.cuda(), gy.cuda(), fused=True)
    assert (route_off, route_on) == ("loop", "loop") and torch.equal(out_on, out_off)
    _, route_valid = _run(m, x.cuda(), trees[1:].cuda().repeat(2, 1, 1), gy.cuda())
    _, route_cpu = _run(cpu, x, trees, gy)
    assert (route_valid, route_cpu) == ("fused", "loop")
