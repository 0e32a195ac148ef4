"""Shared model, inputs and teacher-forced trajectory of the native beam-search decoding tests
(test_beam_decode_cpu.py, test_beam_decode_gpu.py).

The model is the smallest Translation Transformer with two decoder layers. Its embedding is scaled by 0.1: with the raw
random-init weights the beams never reorder after step 0 (every composed parent index is the identity), so an
end-to-end run would say nothing about the cache reorder; with the scaling every sentence reorders in several of its
8 steps.

The teacher-forced trajectory fixes the tokens and a parent map per step (drawn within each sentence's beams, with
duplicates), so the native state and the Table path can be driven through the same discrete history and compared
by their logits alone, without any dependence on which near-tied candidate a number format prefers.
"""
import contextlib

import pytest
import torch

from bigdl_amd import nn
from bigdl_amd.ops import attention as att_ops
from bigdl_amd.utils.random_generator import RNG
from bigdl_amd.utils.table import T

VOCAB, BEAM, MAXLEN, LAYERS, B = 32, 3, 8, 2, 8


def make_model(eos, hidden=64, heads=2):
    RNG.setSeed(1)
    torch.manual_seed(1)
    bs = nn.SequenceBeamSearch(VOCAB, BEAM, 0.6, MAXLEN, eos, 0.0, LAYERS, hidden)
    tr = nn.Transformer(VOCAB, hidden, heads, 2 * hidden, LAYERS, 1.0, 1.0, 1.0, withShareWeightsLinear=True,
                        transformerType=nn.Translation, beamSearch=bs).evaluate()
    tr.embedding.weight.data.mul_(0.1)
    return tr


def make_src(Ls):
    src = torch.randint(3, 33, (B, Ls)).float()
    for b in range(B):
        src[b, Ls - b % 3:] = 0
    return src


@contextlib.contextmanager
def native(on):
    att_ops.set_decode_native(on)
    try:
        yield
    finally:
        att_ops.set_decode_native(None)


def trajectory(seed=7):
    """tokens [B * BEAM, MAXLEN + 1] (column 0 is the start padding) and MAXLEN parent maps [B, BEAM]."""
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(1, VOCAB + 1, (B * BEAM, MAXLEN + 1), generator=g).float()
    tok[:, 0] = 0.0
    parents = []
    for _ in range(MAXLEN):
        p = torch.randint(0, BEAM, (B, BEAM), generator=g)
        p[0] = torch.tensor([0, 0, 2])
        parents.append(p)
    return tok, parents


def _flat_parent(p, dev):
    return ((torch.arange(B).view(B, 1) * BEAM + p).reshape(-1)).to(dev)


def encode(tr, src):
    res = tr.predictModel.forward(src)
    return res[1], res[2]


def teacher_forced_table(tr, src):
    """The Table path (Transformer.symbols) along the fixed trajectory: list of logits [B * BEAM, VOCAB]."""
    enc, bias = encode(tr, src)
    dev = enc.device
    tok, parents = trajectory()
    tok = tok.to(dev)
    rep = torch.arange(B, device=dev).repeat_interleave(BEAM)
    enc_f, bias_f = enc.index_select(0, rep), bias.index_select(0, rep)
    cache = T()
    for j in range(1, LAYERS + 1):
        cache[f"layer_{j}_k"] = torch.zeros(0, device=dev)
        cache[f"layer_{j}_v"] = torch.zeros(0, device=dev)
    ids = tok[:, :1]
    out = []
    for i in range(MAXLEN):
        logits, cache = tr.symbols(ids, i, MAXLEN, enc_f, bias_f, cache)
        out.append(logits.float().cpu())
        fp = _flat_parent(parents[i], dev)
        for name in list(cache.keys()):
            cache[name] = cache[name].index_select(0, fp)
        ids = torch.cat([ids.index_select(0, fp), tok[:, i + 1:i + 2]], 1)
    return out


def teacher_forced_native(tr, src, guard=None):
    """The native state along the same trajectory. ``guard`` (optional) is a context manager factory entered around
    every state.step / state.reorder call."""
    from bigdl_amd.nn.transformer import _DecodeState

    enc, bias = encode(tr, src)
    dev = enc.device
    tok, parents = trajectory()
    tok = tok.to(dev)
    state = _DecodeState(tr, enc, bias, BEAM, MAXLEN)
    guard = guard or contextlib.nullcontext
    ids = tok[:, :1]
    out = []
    for i in range(MAXLEN):
        with guard():
            logits = state.step(ids, i)
        out.append(logits.float().cpu())
        with guard():
            state.reorder(parents[i].to(dev))
        fp = _flat_parent(parents[i], dev)
        ids = torch.cat([ids.index_select(0, fp), tok[:, i + 1:i + 2]], 1)
    return out


def _boom(*a, **kw):
    raise AssertionError("aten math on the native decode path")


@contextlib.contextmanager
def aten_guard():
    mp = pytest.MonkeyPatch()
    try:
        for name in ("matmul", "softmax", "cat", "gather"):
            mp.setattr(torch, name, _boom)
        yield
    finally:
        mp.undo()
