"""Native incremental decoding of Transformer beam search on the GPU engine (csrc/attn_decode.hip under
nn/transformer.py _DecodeState).

Beam search is discrete and bf16 noise flips near-tied candidates (decision margins of this model are 1e-4 .. 2e-2
in log-prob), so nothing here demands equal token ids between a bf16 GPU path and an fp32 oracle:

* teacher-forced: the native state, today's GPU Table path and the fp32 CPU engine are driven through one fixed
  trajectory of tokens and parent maps (tests/beam_decode_cases.py); the native path's max-abs logit error against the
  CPU engine must be <= 1.5 x the Table path's own. Both GPU paths round identical operands to bf16 and differ in
  accumulation order and in the rounding of P, so their errors should be equal; 1.5 covers the max over a finite
  sample. Measured on an MI355X: profiles/decode_native_errors.txt.
* end to end: every sequence the native search returns is re-scored by one full, non-incremental forward of the fp32
  CPU engine; |score - rescored| must be <= 2 x the same quantity for the Table path's own output. This catches a
  cache that no longer matches its sequence whichever candidate the noise prefers.
"""
import copy
import functools

import pytest
import torch

from bigdl_amd.utils.table import T
from tests.beam_decode_cases import (B, BEAM, MAXLEN, VOCAB, aten_guard, make_model, make_src, native,
                                     teacher_forced_native, teacher_forced_table)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def teacher_forced(hidden):
    tr_cpu = make_model(eos=2.0, hidden=hidden)
    src = make_src(6)
    tr = copy.deepcopy(tr_cpu).to(torch.device("cuda"))
    cpu = teacher_forced_table(tr_cpu, src)
    table = teacher_forced_table(tr, src.cuda())
    nat = teacher_forced_native(tr, src.cuda(), guard=aten_guard)     # aten attention math raises in step / reorder
    torch.cuda.synchronize()
    return nat, table, cpu


@pytest.mark.parametrize("hidden", [64, 128])                         # 2 heads: D = 32 and D = 64
def test_teacher_forced_logit_error_vs_table_path(hidden):
    nat, table, cpu = teacher_forced(hidden)
    assert len(nat) == len(table) == len(cpu) == MAXLEN
    assert all(t.shape == (B * BEAM, VOCAB) and torch.isfinite(t).all() for t in nat)
    e_nat = max((a - c).abs().max().item() for a, c in zip(nat, cpu))
    e_tab = max((a - c).abs().max().item() for a, c in zip(table, cpu))
    print(f"DECODE_TF hidden={hidden} native_vs_fp32={e_nat:.4e} table_vs_fp32={e_tab:.4e} "
          f"ratio={e_nat / e_tab:.3f}")
    assert e_tab > 0
    assert e_nat <= 1.5 * e_tab, (e_nat, e_tab)


def test_step_and_reorder_run_without_aten_attention_math():
    nat, _, _ = teacher_forced(64)             # ran under aten_guard: torch.matmul / softmax / cat / gather raise
    assert len(nat) == MAXLEN


def _rescore(tr_cpu, src, seq):
    """Summed log-probs of seq [B, BEAM, 1 + MAXLEN] under one full forward of the fp32 CPU engine."""
    tgt = seq[:, :, 1:].reshape(B * BEAM, MAXLEN).cpu()
    rep = src.repeat_interleave(BEAM, 0)
    logits = tr_cpu.forward(T(rep, tgt)).float()
    lp = torch.log_softmax(logits, -1).gather(2, (tgt.long() - 1).unsqueeze(2)).squeeze(2)
    return lp.sum(1).view(B, BEAM)


def test_end_to_end_scores_match_a_full_fp32_rescoring():
    tr_cpu = make_model(eos=37.0)              # never produced: the output scores are the raw summed log-probs
    src = make_src(8)
    tr = copy.deepcopy(tr_cpu).to(torch.device("cuda"))
    outs = {}
    for on in (True, False):
        with native(on):
            res = tr.forward(src.cuda())
            bs = tr.beamSearch.output
            outs[on] = (bs[1].clone(), bs[2].clone(), res[1].clone(), res[2].clone())
    torch.cuda.synchronize()
    gaps = {}
    for on, (seq, scores, top_ids, top_scores) in outs.items():
        assert seq.shape == (B, BEAM, MAXLEN + 1) and scores.shape == (B, BEAM)
        assert top_ids.shape == (B, MAXLEN) and top_scores.shape == (B,)
        assert torch.equal(top_ids, seq[:, 0, 1:]) and torch.equal(top_scores, scores[:, 0])
        ids = seq[:, :, 1:]
        assert (ids >= 1).all() and (ids <= VOCAB).all() and (ids == ids.round()).all()
        assert (scores[:, 1:] <= scores[:, :-1]).all()          # non-increasing along the beam axis
        gaps[on] = (scores.cpu() - _rescore(tr_cpu, src, seq)).abs().max().item()
    print(f"DECODE_E2E native_gap={gaps[True]:.4e} table_gap={gaps[False]:.4e}")
    assert gaps[False] > 0
    assert gaps[True] <= 2 * gaps[False], gaps
