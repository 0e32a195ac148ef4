"""The fp64 attention reference of tests/attention_edge_cases.py checked on its own (no GPU): the yardstick E_t is
nonzero, the reference is finite, and the errors the GPU tests are meant to catch (one key too many or too few at a
tile tail, a causal rule off by one) move the exact result by more than the 3 E_t those tests allow."""
import pytest
import torch

from tests.attention_edge_cases import CASES, TENSORS, compute, drop_mask, live_batches, make_bias, reference

IDS = [c.name for c in CASES]


def test_case_list_covers_what_the_kernels_tile_over():
    pairs = {(c.Lq, c.Lk) for c in CASES}
    assert {(1, 1), (17, 65), (65, 17), (64, 64), (130, 129), (63, 129)} <= pairs
    assert {c.Lq for c in CASES} >= {1, 15, 17, 63, 64, 65, 130}
    assert {c.Lk for c in CASES} >= {1, 15, 16, 17, 63, 64, 65, 129}
    for d in (32, 64, 96, 128):
        assert {(65, 65), (17, 129)} <= {(c.Lq, c.Lk) for c in CASES if c.D == d}
    assert all(2 <= c.B * c.H <= 6 for c in CASES)
    assert {(c.Lq, c.Lk) for c in CASES if c.causal} >= {(1, 1), (64, 64), (65, 65), (130, 130), (17, 129), (130, 65)}
    assert {c.p for c in CASES} == {0.0, 0.125, 0.5}
    assert max(c.B * c.H * c.Lq * c.Lk for c in CASES if c.p > 0) >= 100_000


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_is_finite_and_yardstick_nonzero(case):
    exact, E = reference(case)
    for t in TENSORS + ("lse",):
        assert torch.isfinite(exact[t]).all(), t
        assert exact[t].shape[0] == len(live_batches(case))
    for t in TENSORS:
        if t == "o" and case.Lk == 1:
            assert E[t] == 0.0         # a single key: P == 1 exactly, o == v, nothing to round
        else:
            assert E[t] > 0.0, t


@pytest.mark.parametrize("case", [c for c in CASES if c.bias == "none" and not c.causal and c.Lk > 1],
                         ids=lambda c: c.name)
def test_dropping_the_last_key_exceeds_the_allowance(case):
    """A kernel that loses the last key of a tile tail is off by more than 3 E_t in every output tensor."""
    exact, E = reference(case)
    wrong, _ = compute(case, perturb="drop_last_key")
    for t in TENSORS:
        moved = (wrong[t] - exact[t]).abs().max().item()
        assert moved > 3 * E[t] + 1e-6 * exact[t].abs().max().item(), (t, moved, E[t])
        assert moved > 10 * E[t], (t, moved, E[t])      # "far below": an order of magnitude of head room


@pytest.mark.parametrize("case", [c for c in CASES if c.causal and c.Lq > 1], ids=lambda c: c.name)
def test_causal_rule_off_by_one_exceeds_the_allowance(case):
    exact, E = reference(case)
    wrong, _ = compute(case, perturb="hide_diagonal")
    for t in TENSORS:
        moved = (wrong[t] - exact[t]).abs().max().item()
        assert moved > 10 * E[t], (t, moved, E[t])


def test_strided_bias_cases_are_really_strided():
    by = {c.bias: c for c in CASES}
    e = make_bias(by["expand"])
    assert e.stride() == (by["expand"].Lk, 0, 0, 1)
    t = make_bias(by["transposed"])
    assert t.stride(3) == by["transposed"].Lq and t.stride(2) == 1
    s = make_bias(by["slice"])
    assert s.storage_offset() > 0 and s.stride(2) == by["slice"].Lk + 7
    for b in (e, t, s):
        assert not b.is_contiguous()


def test_dropout_mask_matches_its_definition():
    """dropout_mask against a scalar re-statement of the kernel's hash, at indices that cross tile and head
    boundaries, and the kept fraction of the largest case."""
    case = max((c for c in CASES if c.p > 0), key=lambda c: (c.B * c.H * c.Lq * c.Lk, c.p))
    from tests.attention_edge_cases import SEED

    def mix(x):
        x &= 0xFFFFFFFF
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        return x ^ (x >> 16)

    M = drop_mask(case).view(case.B * case.H, case.Lq, case.Lk)
    lo, hi = SEED & 0xFFFFFFFF, SEED >> 32
    assert hi != 0
    for bh, qi, kj in ((0, 0, 0), (0, 63, 64), (1, 64, 63), (3, 129, 128), (5, 65, 1)):
        h = mix((mix((bh * case.Lq + qi) ^ lo) + kj * 0x9E3779B9 + hi) & 0xFFFFFFFF)
        want = 1.0 / (1.0 - case.p) if h >= int(case.p * 2 ** 32) else 0.0
        assert M[bh, qi, kj].item() == pytest.approx(want, rel=1e-6)
    assert M.numel() >= 100_000
    assert abs((M > 0).float().mean().item() - (1 - case.p)) < 0.03
