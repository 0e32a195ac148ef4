"""Native incremental decoding of Transformer beam search on the CPU engine: the plumbing (_DecodeState,
SequenceBeamSearch's single composed reorder, the switch) in fp32, where the state runs the torch math of the decode
ops' signatures. The oracle is the Table path (switch off)."""
import copy
import os

import torch

from bigdl_amd import nn
from bigdl_amd.utils.table import T
from tests.beam_decode_cases import (B, BEAM, MAXLEN, VOCAB, make_model, make_src, native, teacher_forced_native,
                                     teacher_forced_table)


def test_end_to_end_equals_table_path(monkeypatch):
    tr = make_model(eos=2.0)
    src = make_src(6)
    # composed parents of the oracle run, from its three top-k calls per step (2K candidates, K alive, K finished)
    calls = []
    real = torch.topk

    def spy(*a, **kw):
        r = real(*a, **kw)
        calls.append(r[1])
        return r

    with native(False), monkeypatch.context() as mp:
        mp.setattr(torch, "topk", spy)
        tr.forward(src)
        want = [t.clone() for t in (tr.beamSearch.output[1], tr.beamSearch.output[2])]
    assert len(calls) % 3 == 0 and len(calls) >= 6
    ident = torch.arange(BEAM).expand(B, BEAM)
    moved = torch.zeros(B, dtype=torch.bool)
    for s in range(1, len(calls) // 3):
        parent = (calls[3 * s] // VOCAB).gather(1, calls[3 * s + 1])
        moved |= (parent != ident).any(1)
    # the condition that makes this test say something about reorder: every sentence reorders after step 0
    assert moved.all(), moved

    made = []
    from bigdl_amd.nn import transformer as trm

    class Counting(trm._DecodeState):
        def __init__(self, *a, **kw):
            made.append(1)
            super().__init__(*a, **kw)

    with native(True), monkeypatch.context() as mp:
        mp.setattr(trm, "_DecodeState", Counting)
        tr.forward(src)
        got = tr.beamSearch.output
    assert made == [1]                                   # the native state drove the search
    assert got[1].shape == want[0].shape == (B, BEAM, want[0].shape[2])
    assert torch.equal(got[1], want[0])                  # all 3 beams' ids
    assert (got[2] - want[1]).abs().max().item() <= 1e-4


def test_default_is_off_on_the_cpu_engine(monkeypatch):
    from bigdl_amd.nn import transformer as trm
    from bigdl_amd.ops import attention as att_ops

    monkeypatch.delenv("BIGDL_DECODE_NATIVE", raising=False)
    assert att_ops.decode_native(False) is False
    monkeypatch.setenv("BIGDL_DECODE_NATIVE", "1")
    assert att_ops.decode_native(False) is True
    monkeypatch.setenv("BIGDL_DECODE_NATIVE", "0")
    assert att_ops.decode_native(True) is False
    monkeypatch.delenv("BIGDL_DECODE_NATIVE")
    from bigdl_amd.utils.engine import Engine

    try:
        Engine.setProperty("bigdl.decode.native", "1")
        assert att_ops.decode_native(False) is True
    finally:
        att_ops.set_decode_native(None)
    tr = make_model(eos=2.0)
    enc = torch.zeros(2, 3, 64)
    assert tr.beamSearch._native_state(enc, torch.zeros(2, 1, 1, 3)) is None
    assert trm.Transformer.symbols is tr.beamSearch.symbolToLogits.__func__


def test_teacher_forced_logits_match_symbols():
    tr = make_model(eos=2.0)
    src = make_src(6)
    want = teacher_forced_table(tr, src)
    got = teacher_forced_native(tr, src)
    assert len(got) == len(want) == MAXLEN
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape == (B * BEAM, VOCAB)
        assert (g - w).abs().max().item() <= 1e-5, i


def test_user_logit_function_keeps_the_table_path(monkeypatch):
    """The reference fixture of test_transformer_cpu.py with native decoding switched on: a user-supplied
    symbolToLogits function is not the Transformer's own, so the Table path runs and the fixture still holds."""
    from bigdl_amd.nn import transformer as trm

    logits = torch.tensor([0.14, 0.62, 0.02, 0.93, 0.59, 0.48, 0.27, 0.70, 0.11, 0.30, 0.35, 0.15,
                           0.67, 0.39, 0.33, 0.01, 0.44, 0.52, 0.45, 0.23, 0.75, 0.79, 0.26, 0.47]).view(6, 4)
    seen = []

    def fn(ids, i, maxlen, enc, bias, layer):
        seen.append(sorted(layer.keys()))
        out = T()
        for j in range(1, 3):
            out[f"layer_{j}_k"] = torch.rand(6, i + 1, 5)
            out[f"layer_{j}_v"] = torch.rand(6, i + 1, 5)
        return logits, out

    def no_state(*a, **kw):
        raise AssertionError("decode state built for a user-supplied logit function")

    monkeypatch.setattr(trm, "_DecodeState", no_state)
    bs = nn.SequenceBeamSearch(4, 3, 0.0, 10, 2.0, 1.0, 2, 5).setLogitFn(fn)
    with native(True):
        out = bs.forward(T(torch.rand(2, 6, 5), torch.rand(2, 1, 1, 6)))
    seq = torch.tensor([[[1, 2, 1, 1, 1], [1, 4, 2, 1, 1], [1, 4, 4, 2, 1]],
                        [[1, 2, 1, 1, 1], [1, 1, 2, 1, 1], [1, 3, 2, 1, 1]]], dtype=torch.float32)
    score = torch.tensor([[-1.2615868, -2.2131736, -3.1647604], [-1.3734006, -2.4668012, -2.715382]])
    assert torch.equal(out[1], seq)
    assert torch.allclose(out[2], score, atol=1e-5)
    assert seen and all(s == ["layer_1_k", "layer_1_v", "layer_2_k", "layer_2_v"] for s in seen)


def test_no_decode_state_is_left_on_the_module(tmp_path):
    from bigdl_amd.nn import transformer as trm
    from bigdl_amd.nn.module import Module

    tr = make_model(eos=2.0)
    src = make_src(6)
    with native(True):
        want = tr.forward(src)
        want = (want[1].clone(), want[2].clone())

    def reachable(obj, seen, depth=0):
        if id(obj) in seen or depth > 60:
            return False
        seen.add(id(obj))
        if isinstance(obj, trm._DecodeState):
            return True
        if isinstance(obj, (list, tuple)):
            return any(reachable(o, seen, depth + 1) for o in obj)
        if isinstance(obj, dict):
            return any(reachable(o, seen, depth + 1) for o in obj.values())
        d = getattr(obj, "__dict__", None)
        return isinstance(d, dict) and any(reachable(o, seen, depth + 1) for o in d.values())

    assert not reachable(tr, set())
    with native(True):
        twin = copy.deepcopy(tr)
        got = twin.forward(src)
        assert torch.equal(got[1], want[0]) and torch.equal(got[2], want[1])
        p = os.path.join(tmp_path, "translation.bigdl")
        tr.saveModule(p, overWrite=True)
        back = Module.loadModule(p)
        assert not reachable(back, set())
