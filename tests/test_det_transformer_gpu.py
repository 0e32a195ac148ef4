"""Deterministic mode end to end on nn.Transformer: two training runs from one initialisation and one seed end with
bitwise-equal weights (ordered attention dQ, LayerNorm parameter gradients and embedding gradient in fixed order).
Language model: five TrainStep iterations; translation: one forward / backward of an encoder-decoder pair with a
padding mask; and one Attention layer with Lq != Lk (the Translation graph joins source and target on the batch, so
it cannot give unequal lengths). Every test restores the mode it found."""
import copy
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def _report(names, a, b):
    """Which parameters (or gradients) differ between two runs, for the assertion message."""
    return [(n, (x - y).abs().max().item()) for n, x, y in zip(names, a, b) if not torch.equal(x, y)]


@pytest.mark.parametrize("optim", ["adam", "sgd"])
def test_transformer_lm_five_steps_bitwise_reproducible(optim):
    """nn.Transformer(100, 128, 2, 256, 2) as a language model (heads 64 wide, all three dropouts on, shared
    embedding), batch 4 x 130 tokens with padding id 0 on half the rows, the PTB trainer's criterion."""
    from det_check import run_transformer, transformer_lm

    from bigdl_amd.utils.random_generator import RNG

    RNG.setSeed(9)
    base = transformer_lm()
    w1, _ = run_transformer(5, True, base, optim=optim)
    w2, _ = run_transformer(5, True, base, optim=optim)
    assert torch.isfinite(w1).all()
    assert torch.equal(w1, w2), (w1 - w2).abs().max().item()


def _grads_of(model, run):
    """Gradients of a deep copy of ``model`` after ``run(copy)`` from a fixed seed; (names, gradient clones)."""
    from bigdl_amd.utils.random_generator import RNG

    m = copy.deepcopy(model).to("cuda")
    m.training()
    RNG.setSeed(11)
    torch.manual_seed(11)
    m.zeroGradParameters()
    run(m)
    torch.cuda.synchronize()
    ws, gs = m.parameters()
    return [f"{i}:{tuple(g.shape)}" for i, g in enumerate(gs)], [g.detach().clone() for g in gs]


def _twice(model, run):
    from bigdl_amd.ops import native

    saved = native.deterministic()
    native.get()
    native.set_deterministic(True)
    try:
        names, a = _grads_of(model, run)
        _, b = _grads_of(model, run)
    finally:
        native.set_deterministic(saved)
    assert all(torch.isfinite(g).all() for g in a)
    assert any(g.abs().max().item() > 0 for g in a)
    assert not _report(names, a, b), _report(names, a, b)


def test_translation_forward_backward_bitwise_reproducible():
    """One encoder-decoder pair, source rows padded (id 0): padding-mask bias on the encoder self attention and on the
    encoder-decoder attention, causal self attention in the decoder."""
    from bigdl_amd import nn
    from bigdl_amd.utils.random_generator import RNG
    from bigdl_amd.utils.table import T

    RNG.setSeed(10)
    tr = nn.Transformer(100, 128, 2, 256, 1, 0.9, 0.9, 0.9, withShareWeightsLinear=True,
                        transformerType=nn.Translation)
    crit = nn.TimeDistributedCriterion(nn.CrossEntropyCriterion(), sizeAverage=False, dimension=2)
    g = torch.Generator().manual_seed(10)
    src = torch.randint(1, 101, (4, 130), generator=g).float()
    src[0, 100:] = 0.0
    src[2, 60:] = 0.0
    tgt = torch.randint(1, 101, (4, 130), generator=g).float()
    lab = torch.randint(1, 101, (4, 130), generator=g).float()

    def run(m):
        x = T(src.cuda(), tgt.cuda())
        c = copy.deepcopy(crit).to("cuda") if hasattr(crit, "to") else crit
        out = m.forward(x)
        c.forward(out, lab.cuda())
        m.backward(x, c.backward(out, lab.cuda()))

    _twice(tr, run)


def test_attention_layer_unequal_lengths_bitwise_reproducible():
    """Attention(128, 2 heads) with Lq = 50 queries over Lk = 70 keys under a padding bias [B, 1, 1, Lk] and
    attention dropout: the projection weights' gradients (which dQ, dK and dV feed) repeat bit for bit."""
    from bigdl_amd import nn
    from bigdl_amd.utils.random_generator import RNG
    from bigdl_amd.utils.table import T

    RNG.setSeed(12)
    att = nn.Attention(128, 2, 0.9)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(4, 50, 128, generator=g)
    y = torch.randn(4, 70, 128, generator=g)
    bias = torch.zeros(4, 1, 1, 70)
    bias[1, ..., 40:] = -1e9
    bias[3, ..., 65:] = -1e9
    go = torch.randn(4, 50, 128, generator=g)

    def run(m):
        inp = T(x.cuda(), y.cuda(), bias.cuda())
        m.forward(inp)
        m.backward(inp, go.cuda())

    _twice(att, run)
