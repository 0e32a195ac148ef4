"""Fused LARS without a GPU: the fp64 oracle of tests/lars_cases.py against the torch route of LarsProcessor +
LarsSGD on the CPU engine (guards included), the exactness of the exact cases, the plan builder's tables, and the
switch with ``last_route()``."""
import pytest
import torch

from bigdl_amd.ops import lars
from bigdl_amd.optim.methods import LarsSGD
from bigdl_amd.optim.sgd import Default
from bigdl_amd.parallel.processors import LarsProcessor
from tests import lars_cases as lc

F32, F64 = lc.F32, lc.F64


class _Comm:
    def all_reduce_scalar(self, t, op="sum"):
        return t


class _Piece:
    def __init__(self, name, lo, hi, method):
        self.name, self.lo, self.hi, self.method = name, lo, hi, method


class _Step:
    """What LarsProcessor reads of a TrainStep: splits, plan, w, g, comm, device."""

    def __init__(self, pieces, methods, w, g):
        self.splits = [(f"l{ly}", lo, hi, m) for (lo, hi, ly), m in zip(pieces, methods)]
        self.plan = [_Piece(*s) for s in self.splits]
        self.w, self.g, self.comm, self.device = w, g, _Comm(), torch.device("cpu")


def _torch_route(pieces, w, g, v, hp, lr, trust, WD):
    """Today's route on fp64 buffers: the processor's scales, then every method's own ``optimize``."""
    w, g = w.to(F64).clone(), g.to(F64).clone()
    methods = []
    for (lo, hi, _), (wd, mom) in zip(pieces, hp):
        m = LarsSGD(Default(), trust, lr, 0.0, wd, mom)
        m.state["v"] = v[lo:hi].to(F64).clone()
        methods.append(m)
    step = _Step(pieces, methods, w, g)
    LarsProcessor(WD)(step)
    for p in step.plan:
        p.method.optimize(lambda _x, _g=g[p.lo:p.hi]: (0.0, _g), w[p.lo:p.hi])
    vout = torch.zeros_like(w)
    for p in step.plan:
        vout[p.lo:p.hi] = p.method.state["v"]
    return w, vout


# The torch route sums the squares in fp32 (LarsProcessor's acc is fp32): a sum of n squares is off by at most
# n 2^-24 relative, each norm by half of that, the scale by both norms' errors plus its own fp32 roundings (root,
# product, sum, quotient, and the rate's quotient: 5 x 2^-24 each way). Everything after the rate runs in fp64 here.
def _rate_tolerance(n):
    return (n + 10) * 2.0 ** -24


def _check_against_torch_route(pieces, w, g, v, hp, rate_num, WD, lr, trust):
    acc = lc.sums_oracle(w, g, pieces, len(pieces))
    we, ve, _ = lc.update_oracle(w, g, v, pieces, hp, rate_num, acc, WD)
    wt, vt = _torch_route(pieces, w, g, v, hp, lr, trust, WD)
    scale = lc.scale_oracle(acc, WD)
    for k, (lo, hi, layer) in enumerate(pieces):
        wd, mom = hp[k]
        step = (rate_num[k] / float(scale[layer])) * (g[lo:hi].to(F64) + wd * w[lo:hi].to(F64))
        tol = _rate_tolerance(hi - lo) * step.abs() + 1e-300
        nan = torch.isnan(ve[lo:hi])
        assert torch.equal(torch.isnan(vt[lo:hi]), nan), k
        assert bool(((vt[lo:hi] - ve[lo:hi]).abs()[~nan] <= tol[~nan]).all()), k
        assert bool(((wt[lo:hi] - we[lo:hi]).abs()[~nan] <= tol[~nan]).all()), k


def test_oracle_agrees_with_the_torch_route_on_gaussian_layers():
    lr, trust = 0.1, 0.001
    pieces, n, w, g, v, hp, _ = lc.gauss_case(lc.LENGTHS, seed=3)
    rate_num = [lr * trust] * len(pieces)
    _check_against_torch_route(pieces, w, g, v, hp, rate_num, lc.GAUSS_WD, lr, trust)


@pytest.mark.parametrize("name", sorted(lc.guard_cases()))
def test_oracle_agrees_with_the_torch_route_on_the_guards(name):
    w, g, WD, want = lc.guard_cases()[name]
    n = w.numel()
    pieces = [(0, n, 0)]
    acc = lc.sums_oracle(w, g, pieces, 1)
    assert float(lc.scale_oracle(acc, WD)[0]) == want
    v = torch.zeros(n, dtype=F32)
    _check_against_torch_route(pieces, w, g, v, [(1e-4, 0.9)], [0.05], WD, 0.1, 0.5)


def _step_f32(w, g, v, pieces, hp, rate_num, acc, WD):
    """The update in fp32 arithmetic (the scale from fp64, rounded once, as the kernel takes it)."""
    w, v = w.clone(), v.clone()
    scale = lc.scale_oracle(acc.to(F32), WD).to(F32)
    for k, (lo, hi, layer) in enumerate(pieces):
        wd, mom = (torch.tensor(x, dtype=F32) for x in hp[k])
        rate = torch.tensor(rate_num[k], dtype=F32) / scale[layer]
        v[lo:hi] = mom * v[lo:hi] + (g[lo:hi] + wd * w[lo:hi]) * rate
        w[lo:hi] = w[lo:hi] - v[lo:hi]
    return w, v


@pytest.mark.parametrize("WD,betas", lc.EXACT_WD)
def test_exact_cases_are_exact(WD, betas):
    pieces, n, w0, hp, rate_num, steps, exact = lc.exact_run(lc.LENGTHS + (lc.FINISH_SECOND_TRIP,), WD, betas, seed=5)
    assert exact
    w, v = w0.to(F32), torch.zeros(n, dtype=F32)
    for g, acc, we, ve in steps:
        assert lc.is_f32(acc) and float(acc.max()) <= 2.0 ** 24
        assert set(lc.scale_oracle(acc, WD).tolist()) <= {1.0, 2.0, 4.0}
        w, v = _step_f32(w, g.to(F32), v, pieces, hp, rate_num, acc, WD)
        assert torch.equal(w.to(F64), we) and torch.equal(v.to(F64), ve)
    assert bool((steps[-1][2] != w0).any())


def _check_tables(pieces, nlayers):
    tab = lars.build_tables(pieces, nlayers)
    C = lars.CHUNK
    assert C == lc.CHUNK and lars.BLOCK_CAP == lc.BLOCK_CAP
    cover = {}
    for c, (k, s) in enumerate(zip(tab["chunk_piece"], tab["chunk_start"])):
        lo, hi, dv, layer = tab["piece_tab"][k]
        assert (lo, hi, layer) == tuple(pieces[k]) and dv % 4 == 0
        e = min(s + C, hi)
        assert lo <= s < e <= hi and (s - lo) % C == 0            # inside its piece, on the piece's chunk grid
        cover.setdefault(k, []).append((s, e))
        first, end = tab["layer_chunks"][layer]
        assert first <= c < end
    for k, (lo, hi, _) in enumerate(pieces):                        # every piece tiled exactly once
        spans = sorted(cover[k])
        assert spans[0][0] == lo and spans[-1][1] == hi
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    pos = 0
    for layer, (first, end) in enumerate(tab["layer_chunks"]):      # contiguous and ordered
        assert first == pos and end >= first
        assert end - first == lc.chunks_of(pieces, layer)
        pos = end
    assert pos == len(tab["chunk_piece"])
    vr = sorted((lo + dv, hi + dv) for lo, hi, dv, _ in tab["piece_tab"])
    assert vr[0][0] >= 0 and vr[-1][1] <= tab["v_need"] and all(a[1] <= b[0] for a, b in zip(vr, vr[1:]))
    assert tab["max_hi"] == max(p[1] for p in pieces)
    return tab


@pytest.mark.parametrize("base", (0, 1, 2, 3))
def test_plan_tables_tile_every_piece_once(base):
    pieces, _ = lc.layout(lc.LENGTHS + (lc.FINISH_SECOND_TRIP,), base)
    _check_tables(pieces, len(pieces))


def test_plan_tables_of_a_two_rank_split():
    pieces, n = lc.layout(lc.LENGTHS)
    inside = pieces[-1][0] + lc.CHUNK + 17            # inside the last layer, not on its chunk grid
    a, b = lc.split_two(pieces, (pieces[4][0] + 5, pieces[6][1], inside))
    L = len(pieces)
    ta, tb = _check_tables(a, L), _check_tables(b, L)
    layers_a, layers_b = {p[2] for p in a}, {p[2] for p in b}
    assert layers_a & layers_b and layers_a - layers_b and layers_b - layers_a
    empty = [ly for ly in range(L) if ly not in layers_a]
    assert empty and all(ta["layer_chunks"][ly][0] == ta["layer_chunks"][ly][1] for ly in empty)
    assert sum(hi - lo for lo, hi, _ in a + b) == n and tb["max_hi"] == n


def test_plan_builder_rejects_bad_pieces():
    with pytest.raises(ValueError):
        lars.build_tables([(4, 4, 0)], 1)
    with pytest.raises(ValueError):
        lars.build_tables([(0, 4, 1)], 1)


def test_switch_and_last_route(monkeypatch):
    monkeypatch.delenv("BIGDL_LARS_FUSED", raising=False)
    try:
        lars.set_fused(None)
        assert lars.fused(True) == lars.DEFAULT_FUSED and not lars.fused(False)
        monkeypatch.setenv("BIGDL_LARS_FUSED", "0")
        assert not lars.fused(True)
        monkeypatch.setenv("BIGDL_LARS_FUSED", "1")
        assert lars.fused(True) and not lars.fused(False)
        lars.set_fused(False)
        assert not lars.fused(True)                 # set_fused wins over the environment
        lars.set_fused("1")
        assert lars.fused(True)
        from bigdl_amd.utils.engine import Engine

        Engine.setProperty("bigdl.lars.fused", "false")
        assert not lars.fused(True)
        # a CPU tensor takes the per-layer body whatever the switch says
        lars.set_fused(True)
        m = LarsSGD(Default(), 0.5, 0.5, 0.0, 0.0, 0.0)
        x, g = torch.ones(8), torch.ones(8)
        m.optimize(lambda _x: (0.0, g), x)
        assert lars.last_route() == "loop"
        assert torch.equal(x, torch.full((8,), 0.75))      # scale 1, rate 0.25
    finally:
        lars.set_fused(None)
