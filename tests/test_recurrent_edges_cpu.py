"""tests/recurrent_cases.py on its own (no GPU): the tile-rule mirrors against the hand-written tables of what each case
is there for, the fp64 oracles against torch autograd of the plain fp64 recurrences, the bounds against an fp32
evaluation of the same formulas on the host, the Philox mask oracle against a plain-integer Philox, and the
sensitivity of the cases: on the very inputs the GPU tests launch, each planted error that applies to the case must
exceed the per-element bound at some element by at least 4x.

Which planted error applies where: a dropped product and a bf16 ulp need a GEMM operand (none in the first / last
step variants, in the top backward step of a sequence, or in the flat cell; a GRU sequence without h0 has an all-zero
operand at step 0); the peephole error needs peepholes, the masked-row error a mask, the row error more than one
row. The sequence cases are checked at every GEMM of every step on the hand-offs a correct launch would have saved
(host emulation); the forward steps of the LSTM sequences past step 0 are not (their states are bounded by 1 and
their weights unspiked there; step 0 carries the spikes). The dropout and weight-gradient oracles get one planted
error each on small data of their own."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import recurrent_cases as rc  # noqa: E402

BF, F32, F64 = rc.BF, rc.F32, rc.F64
SEP = 4.0          # a planted error must exceed the bound by this factor at some element


# ================================================================================================ mirrors
def test_ksplit_values():
    assert [rc.ksplit(K, 16) for K in (32, 96, 256, 512, 544, 1024, 1088, 2048, 2176, 4096, 8192)] == \
        [1, 1, 1, 2, 1, 4, 2, 8, 4, 16, 16]
    assert rc.ksplit(4096, 8) == 8


@pytest.mark.parametrize("shape", list(rc.LSTM_STEP_SHAPES))
def test_lstm_step_shapes_reach_their_instantiations(shape):
    B, H = shape
    want = rc.LSTM_STEP_SHAPES[shape]
    assert rc.reaches(rc.lstm_fwd_tile(H, B), want["fwd"]) == {}
    assert rc.reaches(rc.lstm_bwd_tile(H, B), want["bwd"]) == {}
    f, b = rc.lstm_fwd_tile(H, B), rc.lstm_bwd_tile(H, B)
    assert f["KS"] * f["ksteps"] * 32 == H and b["KS"] * b["ksteps"] * 32 == 4 * H
    assert 64 * f["waves"] <= 1024 and 64 * f["waves"] >= 256 * f["NB"]
    assert 64 * b["KS"] <= 1024 and 64 * b["KS"] >= 256 * b["NB"] * b["NU"]


def test_lstm_step_shapes_cover_every_branch():
    f = [rc.lstm_fwd_tile(H, B) for B, H in rc.LSTM_STEP_SHAPES]
    b = [rc.lstm_bwd_tile(H, B) for B, H in rc.LSTM_STEP_SHAPES]
    assert {t["NB"] for t in f} == {1, 2} and {(t["NB"], t["NU"]) for t in b} == {(1, 1), (2, 1), (2, 2)}
    assert any(t["groups"] and t["tail"] for t in f) and any(not t["groups"] for t in f)
    assert any(t["groups"] and t["tail"] for t in b) and any(t["groups"] and not t["tail"] for t in b)
    assert {t["pad_waves"] for t in f} >= {0, 1, 3}
    assert {t["KS"] for t in f} >= {1, 2, 3, 5, 8, 16} and {t["KS"] for t in b} == {4, 8, 16}


@pytest.mark.parametrize("shape", list(rc.GRU_STEP_SHAPES))
def test_gru_step_shapes_reach_their_instantiations(shape):
    B, H = shape
    assert rc.reaches(rc.gru_tile(H), rc.GRU_STEP_SHAPES[shape]["K"]) == {}
    assert rc.reaches(rc.gru_tile(2 * H), rc.GRU_STEP_SHAPES[shape]["K2"]) == {}


def test_gru_step_shapes_cover_the_issue():
    assert {B % 16 for B, _ in rc.GRU_STEP_SHAPES} == {1, 15, 0}
    ks = {H for _, H in rc.GRU_STEP_SHAPES} | {2 * H for _, H in rc.GRU_STEP_SHAPES}
    assert ks >= {32, 96, 544, 1024, 2048}


@pytest.mark.parametrize("shape", list(rc.LSTM_SEQ_SHAPES))
def test_lstm_seq_shapes(shape):
    B, H, T = shape
    m = rc.seq_shape(B, H)
    assert m["ok"] and rc.reaches(m, rc.LSTM_SEQ_SHAPES[shape]) == {} and T in (1, 2, 4)
    assert m["full_groups"] * m["Bg"] + (m["last_rows"] if m["live_groups"] > m["full_groups"] else 0) == B


@pytest.mark.parametrize("shape", list(rc.GRU_SEQ_SHAPES))
def test_gru_seq_shapes(shape):
    B, H, T = shape
    m = rc.seq_shape(B, H, gru=True)
    assert m["ok"] and m["NT"] == 1 and rc.reaches(m, rc.GRU_SEQ_SHAPES[shape]) == {}
    assert not rc.seq_shape(129, 256, gru=True)["ok"] and not rc.seq_shape(257, 256)["ok"]


def test_cell_shape_past_one_grid_trip():
    B, H = rc.CELL_SHAPES[-1]
    assert (B - 1) * H <= 8192 * 256 < B * H


# ================================================================================================ helpers of the file
def test_guarded_views_and_canaries():
    v, full, lead = rc.guarded(10, F32, "cpu", off=3)
    assert v.numel() == 10 and lead == 256 + 12 and rc.canaries_ok(full, lead, 40)
    v.fill_(1.0)
    assert rc.canaries_ok(full, lead, 40)
    full[lead - 1] = 0
    assert not rc.canaries_ok(full, lead, 40)


def test_bf16_next_is_one_ulp():
    t = torch.tensor([[8.0, -0.5]], dtype=BF)
    assert float(rc.bf16_next(t, (0, 0))[0, 0]) == 8.0625 and float(rc.bf16_next(t, (0, 1))[0, 1]) == -0.50390625


def test_bf16_half_ulp_is_the_rounding_error_bound():
    y = torch.tensor([0.0, 1.0, 1.9921875, 2.0, 3.0, 0.75, 2.0 ** -20], dtype=F64)
    hu = rc.bf16_half_ulp(y)
    assert hu.tolist() == [0.0, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -7, 2.0 ** -9, 2.0 ** -28]
    x = torch.randn(4096, generator=rc.gen(3)) * 5
    err = (x.to(BF).double() - x.double()).abs()
    assert bool((err <= rc.bf16_half_ulp(x.double().abs())).all())
    assert float((err / (2.0 ** -9 * x.double().abs())).max()) > 1.5      # a fixed 2^-9 relative would not hold


def test_ratio_is_strict_where_the_bound_is_zero():
    w = rc.V(torch.tensor([1.0, 2.0]), torch.tensor([0.0, 0.5]))
    assert rc.ratio(torch.tensor([1.0, 2.25]), w) == 0.5
    assert rc.ratio(torch.tensor([1.0 + 2 ** -20, 2.0]), w) == math.inf
    assert rc.ratio(torch.tensor([float("nan"), 2.0]), w) == math.inf


# ================================================================================================ oracles vs autograd
def _lstm_reference(xg, h0, c0, U, peep, masks, order):
    B, T, G = xg.shape
    H = G // 4
    pi, pf, pg, po = order
    h, c, outs = h0, c0, []
    for t in range(T):
        a = xg[:, t] + h @ U.t()
        blk = [a[:, q * H:(q + 1) * H] for q in range(4)]
        i = torch.sigmoid(blk[pi] + (peep[0] * c if peep else 0))
        f = torch.sigmoid(blk[pf] + (peep[1] * c if peep else 0))
        g = torch.tanh(blk[pg])
        cn = f * c + i * g
        o = torch.sigmoid(blk[po] + (peep[2] * cn if peep else 0))
        hn = o * torch.tanh(cn)
        m = masks[t].to(F64).unsqueeze(1) if masks is not None else 1.0
        c = m * cn + (1 - m) * c
        h = m * hn + (1 - m) * h
        outs.append(m * hn)
    return torch.stack(outs, 1), h, c


@pytest.mark.parametrize("peep,masked,order", [(False, False, rc.PLAIN), (True, False, rc.IFGO), (False, True, rc.IFGO),
                                               (True, True, rc.PLAIN), (True, True, (3, 1, 0, 2))])
def test_lstm_oracles_against_autograd(peep, masked, order):
    """The step oracles chained in fp64 (states passed on unrounded) equal the plain recurrence and its autograd
    gradients: outputs, dg of every step, dc0 and dh0 = dg_0 . U + the carry."""
    B, T, H = 5, 4, 32
    g = rc.gen(11)
    xg, h0, c0 = (torch.randn(s, generator=g, dtype=F64) for s in ((B, T, 4 * H), (B, H), (B, H)))
    U = torch.randn(4 * H, H, generator=g, dtype=F64) / math.sqrt(H)
    pp = tuple(torch.randn(H, generator=g, dtype=F64) * 0.5 for _ in range(3)) if peep else None
    masks = (torch.rand(T, B, generator=g) > 0.35).to(torch.uint8) if masked else None
    if masked:
        masks[0, 1], masks[T - 1, 2], masks[:, 3] = 0, 0, 0      # a masked first step, last step and whole row
    leaves = [t.clone().requires_grad_(True) for t in (xg, h0, c0)]
    ro, rh, rcell = _lstm_reference(leaves[0], leaves[1], leaves[2], U, pp, masks, order)
    go, gh, gc = torch.randn(B, T, H, generator=g, dtype=F64), torch.randn(B, H, generator=g, dtype=F64), \
        torch.randn(B, H, generator=g, dtype=F64)
    ((ro * go).sum() + (rh * gh).sum() + (rcell * gc).sum()).backward()
    h, c, acts, cs = h0, c0, [], []
    for t in range(T):
        o = rc.lstm_fwd({"W16": U, "h16_prev": h, "xg": xg[:, t], "c_prev": c, "peep": pp, "order": order, "KS": 1,
                         "mask": masks[t] if masked else None})
        m = masks[t].bool().unsqueeze(1) if masked else torch.ones(B, 1, dtype=torch.bool)
        assert torch.allclose(o["h"].v, ro[:, t].detach(), rtol=0, atol=1e-13)
        h = torch.where(m, o["h"].v, h)
        c = o["c"].v
        acts.append(o["acts"].v)
        cs.append(c)
    assert torch.allclose(h, rh.detach(), rtol=0, atol=1e-13) and torch.allclose(c, rcell.detach(), rtol=0, atol=1e-13)
    # the gradient of the final h is what a masked last step hands on: it starts the carry (as the host code does)
    dc, carry, dgn = gc, gh.clone(), None
    for t in range(T - 1, -1, -1):
        o = rc.lstm_bwd({"WT16": U.t(), "dg16_next": dgn, "dout": go[:, t], "dh_ext": None,
                         "acts": acts[t], "c_prev": cs[t - 1] if t else c0, "c_t": cs[t], "dc": dc, "carry": carry,
                         "peep": pp, "mask": masks[t] if masked else None, "order": order, "KS": 4})
        # the oracle's forward zeroes the activations of a masked row; its backward must not read them
        assert torch.allclose(o["dg"].v, leaves[0].grad[:, t], rtol=0, atol=1e-12), t
        dc, carry, dgn = o["dc"].v, o["carry"].v, o["dg"].v
    assert torch.allclose(dc, leaves[2].grad, rtol=0, atol=1e-12)
    assert torch.allclose(dgn @ U + carry, leaves[1].grad, rtol=0, atol=1e-12)


def test_gru_oracles_against_autograd():
    B, T, H = 5, 4, 32
    g = rc.gen(12)
    xg, h0 = torch.randn(B, T, 3 * H, generator=g, dtype=F64), torch.randn(B, H, generator=g, dtype=F64)
    Urz = torch.randn(2 * H, H, generator=g, dtype=F64) / math.sqrt(H)
    Un = torch.randn(H, H, generator=g, dtype=F64) / math.sqrt(H)
    lx, lh = xg.clone().requires_grad_(True), h0.clone().requires_grad_(True)
    h, outs = lh, []
    for t in range(T):
        rz = torch.sigmoid(lx[:, t, :2 * H] + h @ Urz.t())
        r, z = rz[:, :H], rz[:, H:]
        n = torch.tanh(lx[:, t, 2 * H:] + (r * h) @ Un.t())
        h = (1 - z) * n + z * h
        outs.append(h)
    ro = torch.stack(outs, 1)
    go, gh = torch.randn(B, T, H, generator=g, dtype=F64), torch.randn(B, H, generator=g, dtype=F64)
    ((ro * go).sum() + (h * gh).sum()).backward()
    hp, saved = h0, []
    for t in range(T):
        rz = rc.gru_fwd_rz(Urz, hp, xg[:, t], 1)
        o = rc.gru_fwd_n(Un, rz["r"].v * hp, xg[:, t], rz["z"].v, hp, 1)
        assert torch.allclose(o["h"].v, ro[:, t].detach(), rtol=0, atol=1e-13)
        saved.append((rz["r"].v, rz["z"].v, o["n"].v, hp))
        hp = o["h"].v
    dhp, drz = gh, None
    for t in range(T - 1, -1, -1):
        r, z, n, hprev = saved[t]
        o = rc.gru_bwd_h(Urz.t(), drz, dhp, go[:, t], z, n, hprev, 1)
        o2 = rc.gru_bwd_r(Un.t(), o["dn"].v, o["dhp"], r, hprev, 1)
        dx = torch.cat([o2["dr"].v, o["dz"].v, o["dn"].v], 1)
        assert torch.allclose(dx, lx.grad[:, t], rtol=0, atol=1e-12), t
        dhp, drz = o2["dhp"].v, torch.cat([o2["dr"].v, o["dz"].v], 1)
    assert torch.allclose(rc.gru_bwd_h0(Urz.t(), drz, dhp, 1)["dh0"].v, lh.grad, rtol=0, atol=1e-12)


# ================================================================================================ bounds vs host fp32
def test_bounds_hold_for_an_fp32_evaluation_on_the_host():
    """The same formulas in torch fp32 on the host (its own sum order, its own sigmoid / tanh) stay inside the bounds:
    the bounds are not so tight that a correct fp32 evaluation fails them."""
    for (B, H), variant in (((5, 96), "peep"), ((17, 160), "plain"), ((16, 544), "peep_mask")):
        inp = rc.lstm_fwd_inputs(B, H, variant)
        o = rc.lstm_fwd(inp)
        x = inp["xg"].reshape(B, 4, H)
        pre = (inp["h16_prev"].float() @ inp["W16"].float().t()).reshape(B, 4, H)
        pi, pf, pg, po = inp["order"]
        cp = inp["c_prev"]
        w = inp.get("peep") or (0.0, 0.0, 0.0)
        i = torch.sigmoid(pre[:, pi] + x[:, pi] + w[0] * cp)
        f = torch.sigmoid(pre[:, pf] + x[:, pf] + w[1] * cp)
        g = torch.tanh(pre[:, pg] + x[:, pg])
        c = f * cp + i * g
        og = torch.sigmoid(pre[:, po] + x[:, po] + w[2] * c)
        h = og * torch.tanh(c)
        valid = inp["mask"].bool() if inp.get("mask") is not None else torch.ones(B, dtype=torch.bool)
        assert rc.ratio(c[valid], o["c"].rows(valid)) <= 1.0 and rc.ratio(h[valid], o["h"].rows(valid)) <= 1.0
        assert rc.ratio(i[valid], rc.V(o["acts"].v[valid, pi * H:(pi + 1) * H], o["acts"].e[valid, pi * H:(pi + 1) * H])) <= 1.0
        assert rc.ratio(og[valid], rc.V(o["acts"].v[valid, po * H:(po + 1) * H], o["acts"].e[valid, po * H:(po + 1) * H])) <= 1.0
    for (B, H), variant in (((5, 96), "peep"), ((17, 160), "plain")):
        inp = rc.lstm_bwd_inputs(B, H, variant)
        o = rc.lstm_bwd(inp)
        a = inp["acts"].reshape(B, 4, H)
        pi, pf, pg, po = inp["order"]
        ig, fg, gg, og = a[:, pi], a[:, pf], a[:, pg], a[:, po]
        dh = inp["dout"] + inp["dh_ext"] + inp["dg16_next"].float() @ inp["WT16"].float().t()
        if inp.get("carry") is not None:
            dh = dh + inp["carry"]
        w = inp.get("peep") or (0.0, 0.0, 0.0)
        tc = torch.tanh(inp["c_t"])
        dog = dh * tc * og * (1 - og)
        dcv = dh * og * (1 - tc * tc) + inp["dc"] + dog * w[2]
        di = dcv * gg * ig * (1 - ig)
        df = dcv * inp["c_prev"] * fg * (1 - fg)
        dgg = dcv * ig * (1 - gg * gg)
        dcp = dcv * fg + di * w[0] + df * w[1]
        dg = torch.zeros(B, 4, H)
        dg[:, pi], dg[:, pf], dg[:, pg], dg[:, po] = di, df, dgg, dog
        assert rc.ratio(dg.reshape(B, 4 * H), o["dg"]) <= 1.0 and rc.ratio(dcp, o["dc"]) <= 1.0


# ================================================================================================ sensitivity
def _excess(clean, faulty):
    return max(rc.ratio(faulty[k].v, clean[k]) for k in clean)


def _rows(d, rows):
    return {k: v.rows(rows) for k, v in d.items()}


def _probe(B, mask):
    for b in rc.edge_rows(B):
        if mask is None or bool(mask[b]):
            return b
    return None


def _assert_separated(found, tag):
    assert found, tag
    for name, x in found.items():
        print(f"RECURRENT_SENS|{tag}|{name}|{x:.4g}")
    low = {n: x for n, x in found.items() if not x >= SEP}
    assert not low, (tag, low)


def _lstm_faults(inp, oracle, akey, wkey, K):
    """Every planted error that applies to the case -> the largest |faulty - oracle| / bound over its outputs."""
    B = inp["B"]
    mask = inp.get("mask")
    clean = oracle(inp)
    found = {}
    b = _probe(B, mask)
    if b is not None and inp.get(akey) is not None:
        k1, _ = rc.spike_cols(b, K)
        W = inp[wkey].clone()
        W[0, k1] = 0
        found["one k-term dropped"] = _excess(_rows(clean, [b]), oracle(rc.take_rows({**inp, wkey: W}, [b])))
        A = rc.bf16_next(inp[akey], (b, k1))
        found["one bf16 ulp on a state operand"] = _excess(_rows(clean, [b]), oracle(rc.take_rows({**inp, akey: A}, [b])))
    if b is not None:
        o = list(inp["order"])
        o[0], o[1] = o[1], o[0]
        found["two gate blocks swapped"] = _excess(_rows(clean, [b]), oracle(rc.take_rows({**inp, "order": tuple(o)}, [b])))
    if B > 1:
        e = 16 if B > 16 else B - 1
        found["row past a tile edge takes row 0"] = _excess(_rows(clean, [e]), _rows(clean, [0]))
    if mask is not None:
        r = rc.masked_rows(B)[0]
        m = mask.clone()
        m[r] = 1
        found["masked row advanced"] = _excess(_rows(clean, [r]), oracle(rc.take_rows({**inp, "mask": m}, [r])))
    return found, clean, b


@pytest.mark.parametrize("variant", rc.LSTM_FWD_VARIANTS)
@pytest.mark.parametrize("shape", list(rc.LSTM_STEP_SHAPES))
def test_lstm_fwd_step_cases_separate_the_planted_errors(shape, variant):
    B, H = shape
    inp = rc.lstm_fwd_inputs(B, H, variant)
    found, clean, b = _lstm_faults(inp, rc.lstm_fwd, "h16_prev", "W16", H)
    if inp.get("peep") is not None and b is not None:
        found["peephole on c_t taken from c_{t-1}"] = _excess(
            _rows(clean, [b]), rc.lstm_fwd(rc.take_rows(inp, [b]), peep_o_from_prev=True))
    if B > 1 or inp.get("mask") is None:
        assert "two gate blocks swapped" in found
    if variant in ("plain", "peep", "mask", "peep_mask") and b is not None:
        assert {"one k-term dropped", "one bf16 ulp on a state operand"} <= set(found)
    if variant in ("peep", "peep_mask") and b is not None:
        assert "peephole on c_t taken from c_{t-1}" in found
    if variant in ("mask", "peep_mask", "mask_first"):
        assert "masked row advanced" in found
    # the pre-activations reach the saturated end of tanh_f
    if variant == "plain":
        a = inp["xg"].to(F64) + inp["h16_prev"].to(F64) @ inp["W16"].to(F64).t()
        assert float(a.abs().max()) >= (6.0 if B * H >= 480 else 3.0)
    _assert_separated(found, f"lstm_fwd B{B} H{H} {variant}")


@pytest.mark.parametrize("variant", rc.LSTM_BWD_VARIANTS)
@pytest.mark.parametrize("shape", list(rc.LSTM_STEP_SHAPES))
def test_lstm_bwd_step_cases_separate_the_planted_errors(shape, variant):
    B, H = shape
    inp = rc.lstm_bwd_inputs(B, H, variant)
    found, clean, b = _lstm_faults(inp, rc.lstm_bwd, "dg16_next", "WT16", 4 * H)
    if variant != "last" and b is not None:
        assert {"one k-term dropped", "one bf16 ulp on a state operand"} <= set(found)
    if variant in ("mask", "peep_mask"):
        assert "masked row advanced" in found
    _assert_separated(found, f"lstm_bwd B{B} H{H} {variant}")


@pytest.mark.parametrize("mode", range(5))
@pytest.mark.parametrize("variant", rc.GRU_VARIANTS)
@pytest.mark.parametrize("shape", list(rc.GRU_STEP_SHAPES))
def test_gru_step_cases_separate_the_planted_errors(shape, variant, mode):
    B, H = shape
    gi = rc.gru_inputs(B, H, variant)
    akey, wkey = rc.GRU_MODE_OPERAND[mode]
    K = gi[wkey].shape[1]
    clean = rc.gru_mode(gi, mode)
    found = {}
    b = rc.edge_rows(B)[-1]
    if gi.get(akey) is not None:
        k1, _ = rc.spike_cols(b, K)
        W = gi[wkey].clone()
        W[0, k1] = 0
        found["one k-term dropped"] = _excess(_rows(clean, [b]), rc.gru_mode(rc.take_rows({**gi, wkey: W}, [b]), mode))
        A = rc.bf16_next(gi[akey], (b, k1))
        found["one bf16 ulp on a state operand"] = _excess(_rows(clean, [b]), rc.gru_mode(rc.take_rows({**gi, akey: A}, [b]), mode))
    if mode == 0:
        found["two gate blocks swapped"] = _excess(clean, {"r": clean["z"], "z": clean["r"]})
    if B > 1:
        e = 16 if B > 16 else B - 1
        found["row past a tile edge takes row 0"] = _excess(_rows(clean, [e]), _rows(clean, [0]))
    if not found:
        assert B == 1 and gi.get(akey) is None      # one row, no GEMM: nothing to plant
        return
    _assert_separated(found, f"gru mode{mode} B{B} H{H} {variant}")


def _best_term(A, W, rows):
    """(b, j, k) of the product A[b][k] W[j][k] that is largest against the sum of the magnitudes of its dot product
    (what its chain bound is proportional to), over the batch rows ``rows``."""
    best = (-1.0, None)
    a64, w64 = A.to(F64).abs(), W.to(F64).abs()
    for b in rows:
        t = (a64[b].unsqueeze(0) * w64) / (a64[b].unsqueeze(0) * w64).sum(1, keepdim=True).clamp_min(1e-300)
        i = int(t.argmax())
        if float(t.reshape(-1)[i]) > best[0]:
            best = (float(t.reshape(-1)[i]), (b, i // t.shape[1], i % t.shape[1]))
    return best[1]


def _gemm_faults(inp, oracle, akey, wkey, B):
    """One dropped product and one bf16 ulp on one operand of the GEMM ``inp[akey] . inp[wkey]^T``, planted where
    the product is largest against its dot product, on the case's own operands."""
    clean = oracle(inp)
    b, j, k = _best_term(inp[akey], inp[wkey], rc.edge_rows(B))
    W = inp[wkey].clone()
    W[j, k] = 0
    return {"one k-term dropped": _excess(_rows(clean, [b]), oracle(rc.take_rows({**inp, wkey: W}, [b]))),
            "one bf16 ulp on a state operand": _excess(
                _rows(clean, [b]), oracle(rc.take_rows({**inp, akey: rc.bf16_next(inp[akey], (b, k))}, [b])))}, clean


@pytest.mark.parametrize("shape", list(rc.LSTM_SEQ_SHAPES))
def test_lstm_seq_cases_separate_the_planted_errors(shape):
    """Step 0 of the forward on the given (spiked) inputs, and every backward step and the dh0 round on the hand-offs
    a correct launch would have saved (the host emulation), with the optional arguments the GPU case leaves out left
    out here too. The top backward step has no GEMM: gate blocks and rows only."""
    B, H, T = shape
    si = rc.lstm_seq_inputs(B, H, T)
    saved = rc.emulate_lstm_seq(si)
    inp = {**rc.lstm_seq_fwd_step(si, saved, 0), "B": B}
    found, _, _ = _lstm_faults(inp, rc.lstm_fwd, "h16_prev", "W16", H)
    _assert_separated(found, f"lstm_seq_fwd B{B} H{H} T{T} step0")
    for t in range(T - 1, -1, -1):
        inp = {**saved["bwd_inputs"][t], "B": B}
        if inp["dg16_next"] is not None:
            found, clean = _gemm_faults(inp, rc.lstm_bwd, "dg16_next", "WT16", B)
        else:
            found, clean = {}, rc.lstm_bwd(inp)
        o = list(inp["order"])
        o[0], o[1] = o[1], o[0]
        found["two gate blocks swapped"] = _excess(_rows(clean, [0]), rc.lstm_bwd(rc.take_rows({**inp, "order": tuple(o)}, [0])))
        if B > 1:
            e = 16 if B > 16 else B - 1
            found["row past a tile edge takes row 0"] = _excess(_rows(clean, [e]), _rows(clean, [0]))
        _assert_separated(found, f"lstm_seq_bwd B{B} H{H} T{T} step{t}")
    h0 = {"dg16_next": saved["dg16"][0], "WT16": si["W16"].t().contiguous()}
    found, _ = _gemm_faults(h0, lambda d: {"dh0": rc.dot(d["dg16_next"], d["WT16"], rc.SEQ_BWD_KS, [])}, "dg16_next",
                            "WT16", B)
    _assert_separated(found, f"lstm_seq_bwd B{B} H{H} T{T} dh0")


@pytest.mark.parametrize("shape", list(rc.GRU_SEQ_SHAPES))
def test_gru_seq_cases_separate_the_planted_errors(shape):
    """Every GEMM of every step of the persistent GRU (FWD_RZ and FWD_N of each forward step, BWD_H and BWD_R of each
    backward step, the dh0 round) on the case's own inputs and the hand-offs a correct launch would have saved. A GEMM
    whose operand is absent or all zero (step 0 with h0 = None, BWD_H of the top step) has no product to plant in."""
    B, H, T = shape
    si = rc.gru_seq_inputs(B, H, T)
    saved = rc.emulate_gru_seq(si)
    stages = [(m, t, {**rc.gru_seq_fwd_step(si, saved, t), "B": B}) for t in range(T) for m in (0, 1)]
    stages += [(m, t, {**gi, "B": B}) for m, t, gi in saved["bwd_inputs"]]
    planted = 0
    for mode, t, gi in stages:
        akey, wkey = rc.GRU_MODE_OPERAND[mode]
        tag = f"gru_seq mode{mode} B{B} H{H} T{T} step{t}"
        if gi.get(akey) is None or not bool(gi[akey].to(F32).abs().sum() > 0):
            assert (mode in (0, 1) and t == 0 and si["h0"] is None) or (mode == 2 and t == T - 1), tag
            found, clean = {}, rc.gru_mode(gi, mode)
        else:
            gi = {**gi, wkey: gi[wkey].contiguous()}
            found, clean = _gemm_faults(gi, lambda d: rc.gru_mode(d, mode), akey, wkey, B)
            planted += 1
        if mode == 0:
            found["two gate blocks swapped"] = _excess(clean, {"r": clean["z"], "z": clean["r"]})
        if B > 1:
            found["row past a tile edge takes row 0"] = _excess(_rows(clean, [B - 1]), _rows(clean, [0]))
        if found:
            _assert_separated(found, tag)
    assert planted >= 4 * T - (2 if si["h0"] is None else 0)


@pytest.mark.parametrize("shape", rc.CELL_SHAPES[:2] + ((17, 1024),))
def test_cell_cases_separate_the_planted_errors(shape):
    """The flat cell has no GEMM and no mask: two gate blocks swapped and a row taking row 0's data, on the inputs
    of ``cell_inputs`` (the 2049 x 1024 case draws from the same generator; 17 rows of it are enough here)."""
    B, H = shape
    ci = rc.cell_inputs(B, H)
    swap = torch.cat([ci["gates"][:, 2 * H:3 * H], ci["gates"][:, H:2 * H], ci["gates"][:, :H], ci["gates"][:, 3 * H:]], 1)
    clean = rc.cell_fwd(ci)
    found = {"two gate blocks swapped": _excess(clean, rc.cell_fwd({**ci, "gates": swap})),
             "row past a tile edge takes row 0": _excess(_rows(clean, [B - 1]), _rows(clean, [0]))}
    _assert_separated(found, f"cell_fwd B{B} H{H}")
    aswap = torch.cat([ci["acts"][:, 2 * H:3 * H], ci["acts"][:, H:2 * H], ci["acts"][:, :H], ci["acts"][:, 3 * H:]], 1)
    clean = rc.cell_bwd(ci)
    found = {"two gate blocks swapped": _excess(clean, rc.cell_bwd({**ci, "acts": aswap})),
             "row past a tile edge takes row 0": _excess(_rows(clean, [B - 1]), _rows(clean, [0]))}
    _assert_separated(found, f"cell_bwd B{B} H{H}")


# ================================================================================================ Philox oracle
def _philox_ref(ctr, key):
    """Philox-4x32-10 in plain Python integers on a full 4-word counter and 2-word key (Salmon et al., SC'11)."""
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def test_philox_known_answers_and_the_high_counter_word():
    """The plain-integer Philox against the three published known-answer vectors of Random123 (zeros, all ones, digits
    of pi); the numpy oracle (64-bit counter in the two low words, as the kernel uses it) against it at counters below,
    at and above 2^32 and with keys that use both words."""
    import numpy as np

    f = 0xFFFFFFFF
    assert _philox_ref([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert _philox_ref([f, f, f, f], [f, f]) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert _philox_ref([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    ctrs = [0, 5, (1 << 32) - 1, 1 << 32, (1 << 32) + 7, (1 << 40) + 3, (1 << 63) + 11]
    for seed in (0, 0x1234567887654321, 0xFFFFFFFF00000001):
        got = rc._philox_np(seed, np.array(ctrs, dtype=np.uint64))
        for i, c in enumerate(ctrs):
            want = _philox_ref([c & f, c >> 32, 0, 0], [seed & f, seed >> 32])
            assert [int(w[i]) for w in got] == want, (seed, c)


def test_drop_keep_layout_offsets_and_high_word():
    """The keep mask draws one Philox block per 4 consecutive element ids, id = ((g T + t) B + b) K + k + off: against
    the plain-integer Philox element by element, at offset 0, at a later step's offset, and at an offset whose ids
    straddle 2^34 (the block counter passes 2^32 into its high word)."""
    B, T, K, p, seed = 2, 1, 8, 0.5, 0x1234567887654321
    p32 = float(torch.tensor(p, dtype=F32))
    for off in (0, 3 * 4 * B * K, (1 << 34) - 4 * ((2 * T * B * K) // 4)):
        keep = rc.drop_keep(seed, off, B, T, K, p)
        assert keep.shape == (4, T, B, K)
        ids = [off + i for i in range(4 * T * B * K)]
        assert off < (1 << 34) or (ids[0] >> 2) < (1 << 32) <= (ids[-1] >> 2)
        for i, e in zip(range(keep.numel()), ids):
            w = _philox_ref([(e >> 2) & 0xFFFFFFFF, e >> 34, 0, 0], [seed & 0xFFFFFFFF, seed >> 32])[e & 3]
            assert bool(keep.reshape(-1)[i]) == ((w >> 8) / 16777216.0 >= p32), (off, i)
    k0 = rc.drop_keep(1234567, 0, 5, 3, 12, 0.3)
    assert 0.6 < float(k0.float().mean()) < 0.8
    k8 = rc.drop_keep(1234567, 8, 5, 3, 12, 0.3)
    assert torch.equal(k8.reshape(-1)[:-8], k0.reshape(-1)[8:]) and not torch.equal(k8, k0)


def test_drop_oracles():
    g = rc.gen(5)
    B, T, K, Kp = 3, 2, 8, 16
    x = torch.randn(B, T, K, generator=g)
    keep = rc.drop_keep(77, 4, B, T, K, 0.5)
    y = rc.drop_rep_oracle(x, keep, 2.0, Kp, True)
    assert y.shape == (4, T * B, Kp) and y.dtype == BF
    yv = y.float().reshape(4, T, B, Kp)
    assert bool((yv[..., K] == 1).all()) and bool((yv[..., K + 1:] == 0).all())
    assert torch.equal(yv[..., :K] != 0, keep)
    assert torch.equal(yv[..., :K][keep], (x * 2.0).to(BF).float().permute(1, 0, 2).expand(4, T, B, K)[keep])
    dy = torch.randn(4, T * B, K, generator=g)
    add = torch.randn(B, T, K, generator=g)
    o = rc.drop_rep_bwd_oracle(dy, keep, 2.0, add)
    ref = add.double() + (dy.double().reshape(4, T, B, K) * keep * 2.0).sum(0).permute(1, 0, 2)
    assert torch.allclose(o.v, ref, rtol=0, atol=1e-14) and bool((o.e > 0).all())
    # planted: a dropped element passed through, the mask of another gate
    bad = rc.drop_rep_bwd_oracle(dy, torch.roll(keep, 1, 0), 2.0, add)
    assert rc.ratio(bad.v, o) >= SEP


def test_wgrad_oracle_separates_a_dropped_row():
    T, B, H = rc.WGRAD_SHAPES[0]
    g = rc.gen(6)
    dg16 = (torch.randn(T, B, 4 * H, generator=g) * 0.1).to(BF)
    h16 = (torch.randn(T, B, H, generator=g) * 0.5).to(BF)
    o = rc.wgrad_oracle(dg16, h16)
    d2 = dg16.clone()
    d2[T - 1, B - 1] = 0
    assert rc.ratio(rc.wgrad_oracle(d2, h16).v, o) >= SEP
