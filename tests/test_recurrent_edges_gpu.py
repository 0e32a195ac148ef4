"""The recurrent kernels, each through its own binding, one step at a time against the fp64 oracles of
tests/recurrent_cases.py on exactly the operands the kernel used: lstm_fwd_step / lstm_bwd_step (csrc/lstm.hip),
gru_step modes 0-4 (csrc/gru.hip), the persistent lstm_seq_fwd / lstm_seq_bwd (fp32 and bf16 I/O) and gru_seq_fwd /
gru_seq_bwd (csrc/lstm_seq.hip) by induction over their saved hand-offs, the flat lstm_cell_fwd / lstm_cell_bwd,
lstm_drop_rep / lstm_drop_rep_bwd (csrc/lstm_drop.hip) and the recurrent weight gradient.

* bounded legs: |kernel - oracle| / bound per element, cap 1; the largest ratios measured on an MI355X and the allowed
  values taken from them (``ALLOWED``, 2 x measured rounded up, never above the cap) are in
  profiles/recurrent_edge_errors.txt;
* exact legs (bf16 twins of fp32 outputs, masked rows, hT, bf16-I/O outputs, dropout output, sentinels) are held to
  equality;
* every tensor a binding writes is a view inside a larger allocation of sentinel bytes (``_Arena``): a store to a row
  past B or outside the view is seen without leaving the allocation;
* before every launch the mirrors of the cases file assert the instantiation the case is named for.
"""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import recurrent_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu

BF, F32, F64 = rc.BF, rc.F32, rc.F64
DEV = "cuda"

# Allowed largest |kernel - oracle| / bound per leg: 2 x the largest ratio measured on an MI355X, rounded up to two
# significant digits, never above the cap of 1; the same table stands in profiles/recurrent_edge_errors.txt.
LEGS = ("lstm_fwd_acts", "lstm_fwd_c", "lstm_fwd_h", "lstm_bwd_dg", "lstm_bwd_dc", "lstm_bwd_carry",
        "gru_rz", "gru_n", "gru_h", "gru_dn", "gru_dz", "gru_dr", "gru_dhp", "gru_dh0",
        "lstm_seq_acts", "lstm_seq_c", "lstm_seq_h", "lstm_seq_h_bf16", "lstm_seq_dg", "lstm_seq_dg_bf16", "lstm_seq_dc0",
        "lstm_seq_dh0",
        "gru_seq_rz", "gru_seq_n", "gru_seq_h", "gru_seq_dx", "gru_seq_dh0",
        "cell_fwd", "cell_bwd", "drop_bwd", "wgrad")
CAPS = {k: 1.0 for k in LEGS}
ALLOWED = {"lstm_fwd_acts": 1.0, "lstm_fwd_c": 0.95, "lstm_fwd_h": 0.61, "lstm_bwd_dg": 1.0, "lstm_bwd_dc": 1.0,
           "lstm_bwd_carry": 0.039, "gru_rz": 1.0, "gru_n": 0.074, "gru_h": 0.27, "gru_dn": 1.0, "gru_dz": 1.0,
           "gru_dr": 0.061, "gru_dhp": 1.0, "gru_dh0": 0.04, "lstm_seq_acts": 0.022, "lstm_seq_c": 0.014,
           "lstm_seq_h": 0.012, "lstm_seq_h_bf16": 1.0, "lstm_seq_dg": 1.0, "lstm_seq_dg_bf16": 1.0, "lstm_seq_dc0":
           1.0, "lstm_seq_dh0": 0.0062, "gru_seq_rz": 0.51, "gru_seq_n": 0.074, "gru_seq_h": 0.47, "gru_seq_dx": 1.0,
           "gru_seq_dh0": 0.0086, "cell_fwd": 1.0, "cell_bwd": 1.0, "drop_bwd": 0.65, "wgrad": 0.18}
assert set(ALLOWED) == set(CAPS) and all(ALLOWED[k] <= CAPS[k] for k in CAPS)


def _report(name, case, value):
    """Prints one line per measured figure (pytest -s shows them; profiles/recurrent_edge_errors.txt holds their
    maxima) and returns the figure for the assertion at the place of measurement."""
    print(f"RECURRENT|{name}|{case}|{value:.4g}")
    return value


def _n():
    from bigdl_amd.ops import native

    return native.get()


class _Arena:
    """Guarded device views; ``ok()`` after the launches asserts every sentinel byte on both sides of every view."""

    def __init__(self):
        self.items = []

    def new(self, shape, dtype):
        n = 1
        for s in shape:
            n *= s
        v, full, lead = rc.guarded(n, dtype, DEV)
        assert full.data_ptr() % 256 == 0
        self.items.append((full, lead, n * v.element_size()))
        return v.view(shape)

    def put(self, src):
        if src is None:
            return None
        v = self.new(tuple(src.shape), src.dtype)
        v.copy_(src)
        return v

    def ok(self):
        torch.cuda.synchronize()
        return all(rc.canaries_ok(*it) for it in self.items)


def _bound(leg, case, got, want):
    r = _report(leg, case, rc.ratio(got, want))
    assert r <= ALLOWED[leg], (leg, case, rc.worst(got, want))


def _untouched(t):
    """Every byte of the view still holds the sentinel."""
    return bool((t.contiguous().view(torch.uint8) == rc.SENTINEL).all())


def _with_bf16_rounding(v):
    """The bound of a value that is stored as bf16: one round-to-nearest adds half a bf16 ulp of the rounded fp32
    number, which lies within v.e of v.v."""
    return rc.V(v.v, v.e + rc.bf16_half_ulp(v.v.abs() + v.e))


# ================================================================================================== 1. LSTM steps
_STEP_IDS = [f"B{B}-H{H}" for B, H in rc.LSTM_STEP_SHAPES]


@pytest.mark.parametrize("variant", rc.LSTM_FWD_VARIANTS)
@pytest.mark.parametrize("shape", list(rc.LSTM_STEP_SHAPES), ids=_STEP_IDS)
def test_lstm_fwd_step(shape, variant):
    B, H = shape
    C = _n()
    tile = rc.lstm_fwd_tile(H, B)
    assert rc.reaches(tile, rc.LSTM_STEP_SHAPES[shape]["fwd"]) == {}
    inp = rc.lstm_fwd_inputs(B, H, variant)
    assert rc.lstm_general(inp) == (variant not in ("plain", "first"))
    case = f"B{B}-H{H}-{variant}"
    A = _Arena()
    W16, h16p, cp = A.put(inp["W16"]), A.put(inp["h16_prev"]), A.put(inp["c_prev"])
    c_out, h16_out, acts = A.new((B, H), F32), A.new((B, H), BF), A.new((B, 4 * H), F32)
    strided = variant == "plain"           # row-strided xg and h_out (a [B, T, .] tensor's step view)
    if strided:
        xg3 = A.new((B, 2, 4 * H), F32)
        xg3[:, 1].copy_(inp["xg"])
        xg = xg3[:, 1]
        h3 = A.new((B, 2, H), F32)
        h_out = h3[:, 1]
    else:
        xg, h_out = A.put(inp["xg"]), A.new((B, H), F32)
    hst = A.put(inp.get("h_state"))
    peep = [A.put(p) for p in inp["peep"]] if inp.get("peep") is not None else [None] * 3
    mask = A.put(inp.get("mask"))
    C.lstm_fwd_step(W16, h16p, xg, cp, c_out, h_out, h16_out, acts, h_state=hst, pI=peep[0], pF=peep[1], pO=peep[2],
                    mask=mask, order=list(inp["order"]))
    assert A.ok(), case
    if strided:
        assert _untouched(h3[:, 0]) and _untouched(xg3[:, 0])
    o = rc.lstm_fwd(inp)
    _bound("lstm_fwd_acts", case, acts, o["acts"])
    _bound("lstm_fwd_c", case, c_out, o["c"])
    _bound("lstm_fwd_h", case, h_out, o["h"])
    valid = inp["mask"].bool() if inp.get("mask") is not None else torch.ones(B, dtype=torch.bool)
    h16_cpu, h_cpu = h16_out.cpu(), h_out.contiguous().cpu()
    assert rc.same_bits(h16_cpu[valid], rc.rne_bf16(h_cpu[valid])), case
    if hst is not None:
        assert rc.same_bits(hst.cpu()[valid], h_cpu[valid]) and rc.same_bits(hst.cpu()[~valid], inp["h_state"][~valid])
    if not bool(valid.all()):
        m = ~valid
        prev16 = inp["h16_prev"] if inp["h16_prev"] is not None else torch.zeros(B, H, dtype=BF)
        assert rc.same_bits(c_out.cpu()[m], inp["c_prev"][m]), case
        assert rc.same_bits(h16_cpu[m], prev16[m]), case
        assert rc.same_bits(h_cpu[m], torch.zeros_like(h_cpu[m])) and rc.same_bits(acts.cpu()[m], torch.zeros(int(m.sum()), 4 * H))
    # the inputs are read-only
    assert rc.same_bits(W16.cpu(), inp["W16"]) and rc.same_bits(xg.contiguous().cpu(), inp["xg"])


@pytest.mark.parametrize("variant", rc.LSTM_BWD_VARIANTS)
@pytest.mark.parametrize("shape", list(rc.LSTM_STEP_SHAPES), ids=_STEP_IDS)
def test_lstm_bwd_step(shape, variant):
    B, H = shape
    C = _n()
    assert rc.reaches(rc.lstm_bwd_tile(H, B), rc.LSTM_STEP_SHAPES[shape]["bwd"]) == {}
    inp = rc.lstm_bwd_inputs(B, H, variant)
    assert rc.lstm_general(inp) == (variant not in ("plain", "last"))
    case = f"B{B}-H{H}-{variant}"
    A = _Arena()
    WT16, dg16n, dh_ext = A.put(inp["WT16"]), A.put(inp["dg16_next"]), A.put(inp["dh_ext"])
    acts, cp, ct, dc = A.put(inp["acts"]), A.put(inp["c_prev"]), A.put(inp["c_t"]), A.put(inp["dc"])
    dg16_out = A.new((B, 4 * H), BF)
    strided = variant == "plain"           # row-strided dout and dg_out
    if strided:
        d3 = A.new((B, 2, H), F32)
        d3[:, 1].copy_(inp["dout"])
        dout = d3[:, 1]
        g3 = A.new((B, 2, 4 * H), F32)
        dg_out = g3[:, 1]
    else:
        dout, dg_out = A.put(inp["dout"]), A.new((B, 4 * H), F32)
    carry = A.put(inp.get("carry"))
    peep = [A.put(p) for p in inp["peep"]] if inp.get("peep") is not None else [None] * 3
    mask = A.put(inp.get("mask"))
    C.lstm_bwd_step(WT16, dg16n, dout, dh_ext, acts, cp, ct, dc, dg_out, dg16_out, carry=carry, pI=peep[0], pF=peep[1],
                    pO=peep[2], mask=mask, order=list(inp["order"]))
    assert A.ok(), case
    if strided:
        assert _untouched(g3[:, 0]) and _untouched(d3[:, 0])
    o = rc.lstm_bwd(inp)
    _bound("lstm_bwd_dg", case, dg_out, o["dg"])
    _bound("lstm_bwd_dc", case, dc, o["dc"])
    if carry is not None:
        _bound("lstm_bwd_carry", case, carry, o["carry"])
    dg_cpu = dg_out.contiguous().cpu()
    assert rc.same_bits(dg16_out.cpu(), rc.rne_bf16(dg_cpu)), case
    if inp.get("mask") is not None:
        m = ~inp["mask"].bool()
        assert rc.same_bits(dg_cpu[m], torch.zeros(int(m.sum()), 4 * H)) and rc.same_bits(dc.cpu()[m], inp["dc"][m])
        assert rc.same_bits(dg16_out.cpu()[m], torch.zeros(int(m.sum()), 4 * H, dtype=BF))
    if carry is not None:
        v = inp["mask"].bool() if inp.get("mask") is not None else torch.ones(B, dtype=torch.bool)
        assert rc.same_bits(carry.cpu()[v], torch.zeros(int(v.sum()), H)), case
    assert rc.same_bits(acts.cpu(), inp["acts"]) and rc.same_bits(ct.cpu(), inp["c_t"])


# ================================================================================================== 2. GRU steps
_GRU_IDS = [f"B{B}-H{H}" for B, H in rc.GRU_STEP_SHAPES]


@pytest.mark.parametrize("variant", rc.GRU_VARIANTS)
@pytest.mark.parametrize("shape", list(rc.GRU_STEP_SHAPES), ids=_GRU_IDS)
def test_gru_step_modes(shape, variant):
    B, H = shape
    C = _n()
    assert rc.reaches(rc.gru_tile(H), rc.GRU_STEP_SHAPES[shape]["K"]) == {}
    assert rc.reaches(rc.gru_tile(2 * H), rc.GRU_STEP_SHAPES[shape]["K2"]) == {}
    gi = rc.gru_inputs(B, H, variant)
    case = f"B{B}-H{H}-{variant}"
    A = _Arena()
    d = {k: A.put(gi[k]) for k in ("Wrz", "Wn", "WrzT", "WnT", "h16", "rh16", "drz16", "dn16", "xg", "hprev", "dout",
                                   "z", "r", "n")}
    zero_h = torch.zeros(B, H)
    hp_cpu = gi["hprev"] if gi["hprev"] is not None else zero_h
    # mode 0: r, z, (r h)16; the split at j = H
    r, z, rh16 = A.new((B, H), F32), A.new((B, H), F32), A.new((B, H), BF)
    C.gru_step(0, d["h16"], d["Wrz"], B, H, xg=d["xg"], hprev=d["hprev"], r=r, z=z, rh16=rh16)
    assert A.ok(), case
    o = rc.gru_mode(gi, 0)
    _bound("gru_rz", case + "-r", r, o["r"])
    _bound("gru_rz", case + "-z", z, o["z"])
    assert rc.same_bits(rh16.cpu(), rc.rne_bf16(r.cpu() * hp_cpu)), case
    # mode 1: n, h on the given (r h)16 and z
    n, hout, h16out = A.new((B, H), F32), A.new((B, H), F32), A.new((B, H), BF)
    C.gru_step(1, d["rh16"], d["Wn"], B, H, xg=d["xg"], hprev=d["hprev"], z=d["z"], n=n, hout=hout, h16out=h16out)
    assert A.ok(), case
    o = rc.gru_mode(gi, 1)
    _bound("gru_n", case, n, o["n"])
    _bound("gru_h", case, hout, o["h"])
    assert rc.same_bits(h16out.cpu(), rc.rne_bf16(hout.cpu())), case
    # mode 2: dn, dz, the z-path of dhp (in place); the r columns of dx and drz16 stay untouched
    dhp, dx = A.put(gi["dhp"]), A.new((B, 3 * H), F32)
    dn16, drz16 = A.new((B, H), BF), A.new((B, 2 * H), BF)
    C.gru_step(2, d["drz16"], d["WrzT"], B, H, hprev=d["hprev"], z=d["z"], n=d["n"], dout=d["dout"], dhp=dhp, dx=dx,
               dn16=dn16, drz16=drz16)
    assert A.ok(), case
    o2 = rc.gru_mode(gi, 2)
    _bound("gru_dn", case, dx[:, 2 * H:], o2["dn"])
    _bound("gru_dz", case, dx[:, H:2 * H], o2["dz"])
    _bound("gru_dhp", case + "-zpath", dhp, o2["dhp"])
    dx_cpu = dx.cpu()
    assert _untouched(dx[:, :H]) and _untouched(drz16[:, :H])
    assert rc.same_bits(dn16.cpu(), rc.rne_bf16(dx_cpu[:, 2 * H:].contiguous()))
    assert rc.same_bits(drz16.cpu()[:, H:].contiguous(), rc.rne_bf16(dx_cpu[:, H:2 * H].contiguous()))
    # mode 3 on the same buffers, its operand the kernel's own dn16: dr and dhp += r-path, against the fp64 sum of both
    C.gru_step(3, dn16, d["WnT"], B, H, hprev=d["hprev"], r=d["r"], dhp=dhp, dx=dx, drz16=drz16)
    assert A.ok(), case
    o3 = rc.gru_mode({**gi, "dn16": dn16.cpu(), "dhp": o2["dhp"]}, 3)
    _bound("gru_dr", case + "-chained", dx[:, :H], o3["dr"])
    _bound("gru_dhp", case + "-both", dhp, o3["dhp"])
    dx2 = dx.cpu()
    assert rc.same_bits(dx2[:, H:].contiguous(), dx_cpu[:, H:].contiguous())
    assert rc.same_bits(drz16.cpu()[:, :H].contiguous(), rc.rne_bf16(dx2[:, :H].contiguous()))
    # mode 3 alone on the case's spiked dn16
    dhp_b, dx_b, drz_b = A.put(gi["dhp"]), A.new((B, 3 * H), F32), A.new((B, 2 * H), BF)
    C.gru_step(3, d["dn16"], d["WnT"], B, H, hprev=d["hprev"], r=d["r"], dhp=dhp_b, dx=dx_b, drz16=drz_b)
    assert A.ok(), case
    o = rc.gru_mode(gi, 3)
    _bound("gru_dr", case, dx_b[:, :H], o["dr"])
    _bound("gru_dhp", case + "-rpath", dhp_b, o["dhp"])
    assert _untouched(dx_b[:, H:]) and _untouched(drz_b[:, H:])
    # mode 4: dh0 from the case's drz16 and the dhp the kernel left
    dh0 = A.new((B, H), F32)
    dhp_now = dhp.cpu()
    C.gru_step(4, d["drz16"], d["WrzT"], B, H, dhp=dhp, dh0=dh0)
    assert A.ok(), case
    _bound("gru_dh0", case, dh0, rc.gru_mode({**gi, "dhp": dhp_now}, 4)["dh0"])
    assert rc.same_bits(dhp.cpu(), dhp_now)


# ================================================================================================== 3. persistent
@pytest.mark.parametrize("bio", [False, True], ids=["f32io", "bf16io"])
@pytest.mark.parametrize("shape", list(rc.LSTM_SEQ_SHAPES), ids=[f"B{B}-H{H}-T{T}" for B, H, T in rc.LSTM_SEQ_SHAPES])
def test_lstm_seq_by_induction(shape, bio):
    from bigdl_amd.ops import native

    B, H, T = shape
    C = _n()
    m = rc.seq_shape(B, H)
    assert m["ok"] and rc.reaches(m, rc.LSTM_SEQ_SHAPES[shape]) == {}
    if not C.lstm_seq_supported(B, H):
        pytest.skip("the device refuses the shape")
    si = rc.lstm_seq_inputs(B, H, T)       # the optional arguments of LSTM_SEQ_OPT are None in it
    opt = si["opt"]
    case = f"B{B}-H{H}-T{T}-{'bf16' if bio else 'f32'}{'-' + opt if opt else ''}"
    io = BF if bio else F32
    xg_io = si["xg"].to(io)
    native.check_persistent()
    A = _Arena()
    W16, xg, c0 = A.put(si["W16"]), A.put(xg_io), A.put(si["c0"])
    h16 = A.new((T + 1, B, H), BF)
    h16[0].copy_(si["h0_16"])
    out, cs, acts = A.new((B, T, H), io), A.new((T, B, H), F32), A.new((T, B, 4 * H), F32)
    hT = None if opt == "no_hT" else A.new((B, H), F32)
    sync = A.new((int(C.lstm_seq_sync_words()),), torch.int32)
    assert C.lstm_seq_supported(B, H)
    C.lstm_seq_fwd(W16, xg, c0, h16, out, hT, cs, acts, sync)
    assert A.ok(), case
    native.check_persistent()
    saved = {"h16": h16.cpu(), "cs": cs.cpu(), "acts": acts.cpu()}
    out_cpu = out.cpu()
    assert rc.same_bits(saved["h16"][0], si["h0_16"])
    for t in range(T):
        o = rc.lstm_fwd(rc.lstm_seq_fwd_step(si, saved, t, xg=xg_io))
        _bound("lstm_seq_acts", f"{case}-t{t}", saved["acts"][t], o["acts"])
        _bound("lstm_seq_c", f"{case}-t{t}", saved["cs"][t], o["c"])
        if bio:       # the layer output is the bf16 state itself
            assert rc.same_bits(out_cpu[:, t].contiguous(), saved["h16"][t + 1]), (case, t)
            _bound("lstm_seq_h_bf16", f"{case}-t{t}", saved["h16"][t + 1], _with_bf16_rounding(o["h"]))
        else:
            _bound("lstm_seq_h", f"{case}-t{t}", out_cpu[:, t], o["h"])
            assert rc.same_bits(saved["h16"][t + 1], rc.rne_bf16(out_cpu[:, t].contiguous())), (case, t)
        if t == T - 1 and hT is not None:
            if bio:
                _bound("lstm_seq_h", f"{case}-hT", hT, o["h"])
                assert rc.same_bits(rc.rne_bf16(hT.cpu()), saved["h16"][T])
            else:
                assert rc.same_bits(hT.cpu(), out_cpu[:, -1].contiguous()), case
    # backward on the launch's own acts / cs
    dout_io = si["dout"].to(io) if si["dout"] is not None else None
    dhT, dcT = si["dhT"], si["dcT"]
    assert (dout_io is None) == (opt == "no_dout") and (dhT is None) == (dcT is None) == (opt == "no_dhT_dcT")
    dout, dhT_d, dcT_d = A.put(dout_io), A.put(dhT), A.put(dcT)
    dg16, dxg = A.new((T, B, 4 * H), BF), A.new((B, T, 4 * H), io)
    dc0, dh0 = A.new((B, H), F32), A.new((B, H), F32)
    sync2 = A.new((int(C.lstm_seq_sync_words()),), torch.int32)
    C.lstm_seq_bwd(W16, dout, dhT_d, dcT_d, acts, cs, c0, dg16, dxg, dc0, dh0, sync2)
    assert A.ok(), case
    native.check_persistent()
    assert rc.same_bits(acts.cpu(), saved["acts"]) and rc.same_bits(cs.cpu(), saved["cs"])
    saved["dg16"] = dg16.cpu()
    dxg_cpu = dxg.cpu()
    dc = rc.V(dcT if dcT is not None else torch.zeros(B, H))
    for t in range(T - 1, -1, -1):
        o = rc.lstm_bwd(rc.lstm_seq_bwd_step(si, saved, t, dc, dout_io, dhT))
        if bio:       # the input-projection gradient is the bf16 hand-off itself
            assert rc.same_bits(dxg_cpu[:, t].contiguous(), saved["dg16"][t]), (case, t)
            _bound("lstm_seq_dg_bf16", f"{case}-t{t}", saved["dg16"][t], _with_bf16_rounding(o["dg"]))
        else:
            _bound("lstm_seq_dg", f"{case}-t{t}", dxg_cpu[:, t], o["dg"])
            assert rc.same_bits(saved["dg16"][t], rc.rne_bf16(dxg_cpu[:, t].contiguous())), (case, t)
        dc = o["dc"]
    _bound("lstm_seq_dc0", case, dc0, dc)
    _bound("lstm_seq_dh0", case, dh0, rc.dot(saved["dg16"][0], si["W16"].t(), rc.SEQ_BWD_KS, []))


@pytest.mark.parametrize("shape", list(rc.GRU_SEQ_SHAPES), ids=[f"B{B}-H{H}-T{T}" for B, H, T in rc.GRU_SEQ_SHAPES])
def test_gru_seq_by_induction(shape):
    from bigdl_amd.ops import native

    B, H, T = shape
    C = _n()
    m = rc.seq_shape(B, H, gru=True)
    assert m["ok"] and rc.reaches(m, rc.GRU_SEQ_SHAPES[shape]) == {}
    if not C.gru_seq_supported(B, H):
        pytest.skip("the device refuses the shape")
    si = rc.gru_seq_inputs(B, H, T)        # the optional arguments of GRU_SEQ_OPT are None in it
    opt = si["opt"]
    assert (si["h0"] is None) == (opt == "no_h0")
    case = f"B{B}-H{H}-T{T}{'-' + opt if opt else ''}"
    native.check_persistent()
    A = _Arena()
    Wrz, Wn, xg, h0 = A.put(si["Wrz"]), A.put(si["Wn"]), A.put(si["xg"]), A.put(si["h0"])
    h16 = A.new((T + 1, B, H), BF)
    h16[0].copy_(si["h0_16"])
    rh16, gates, out = A.new((T, B, H), BF), A.new((3, T, B, H), F32), A.new((B, T, H), F32)
    sync = A.new((int(C.lstm_seq_sync_words()),), torch.int32)
    assert C.gru_seq_supported(B, H)
    C.gru_seq_fwd(Wrz, Wn, xg, h0, h16, rh16, gates, out, sync)
    assert A.ok(), case
    native.check_persistent()
    saved = {"h16": h16.cpu(), "rh16": rh16.cpu(), "gates": gates.cpu(), "out": out.cpu()}
    for t in range(T):
        gi = rc.gru_seq_fwd_step(si, saved, t)
        o = rc.gru_mode(gi, 0)
        _bound("gru_seq_rz", f"{case}-t{t}-r", saved["gates"][0, t], o["r"])
        _bound("gru_seq_rz", f"{case}-t{t}-z", saved["gates"][1, t], o["z"])
        hp = gi["hprev"] if gi["hprev"] is not None else torch.zeros(B, H)
        assert rc.same_bits(saved["rh16"][t], rc.rne_bf16(saved["gates"][0, t] * hp)), (case, t)
        o = rc.gru_mode(gi, 1)
        _bound("gru_seq_n", f"{case}-t{t}", saved["gates"][2, t], o["n"])
        _bound("gru_seq_h", f"{case}-t{t}", saved["out"][:, t], o["h"])
        assert rc.same_bits(saved["h16"][t + 1], rc.rne_bf16(saved["out"][:, t].contiguous())), (case, t)
    dout_c, dhT_c = si["dout"], si["dhT"]
    assert (dout_c is None) == (opt == "no_dout") and (dhT_c is None) == (opt == "no_dhT")
    dout, dhT = A.put(dout_c), A.put(dhT_c)
    dx, dn16, drz16 = A.new((B, T, 3 * H), F32), A.new((T, B, H), BF), A.new((T, B, 2 * H), BF)
    dh0 = A.new((B, H), F32)
    sync2 = A.new((int(C.lstm_seq_sync_words()),), torch.int32)
    C.gru_seq_bwd(Wrz, Wn, h0, gates, out, dout, dhT, dx, dn16, drz16, dh0, sync2)
    assert A.ok(), case
    native.check_persistent()
    saved["dn16"], saved["drz16"] = dn16.cpu(), drz16.cpu()
    dx_cpu = dx.cpu()
    dhp = rc.V(dhT_c if dhT_c is not None else torch.zeros(B, H))
    for t in range(T - 1, -1, -1):
        gi = rc.gru_seq_bwd_step(si, saved, t, dhp, dout_c)
        o2 = rc.gru_mode(gi, 2)
        _bound("gru_seq_dx", f"{case}-t{t}-dn", dx_cpu[:, t, 2 * H:], o2["dn"])
        _bound("gru_seq_dx", f"{case}-t{t}-dz", dx_cpu[:, t, H:2 * H], o2["dz"])
        assert rc.same_bits(saved["dn16"][t], rc.rne_bf16(dx_cpu[:, t, 2 * H:].contiguous())), (case, t)
        assert rc.same_bits(saved["drz16"][t][:, H:].contiguous(), rc.rne_bf16(dx_cpu[:, t, H:2 * H].contiguous())), (case, t)
        o3 = rc.gru_mode({**gi, "dhp": o2["dhp"]}, 3)
        _bound("gru_seq_dx", f"{case}-t{t}-dr", dx_cpu[:, t, :H], o3["dr"])
        assert rc.same_bits(saved["drz16"][t][:, :H].contiguous(), rc.rne_bf16(dx_cpu[:, t, :H].contiguous())), (case, t)
        dhp = o3["dhp"]
    _bound("gru_seq_dh0", case, dh0, rc.gru_bwd_h0(si["Wrz"].t(), saved["drz16"][0], dhp, rc.GRU_SEQ_KS)["dh0"])


# ================================================================================================== 4. flat cell
@pytest.mark.parametrize("shape", rc.CELL_SHAPES, ids=[f"B{B}-H{H}" for B, H in rc.CELL_SHAPES])
def test_lstm_cell_flat_kernels(shape):
    B, H = shape
    C = _n()
    ci = rc.cell_inputs(B, H)
    variants = [(True, True, True)] + ([(False, False, True), (True, True, False)] if B * H < 4096 else [])
    for with_cp, with_dh, with_dc in variants:
        case = f"B{B}-H{H}-{int(with_cp)}{int(with_dh)}{int(with_dc)}"
        A = _Arena()
        gates, cp = A.put(ci["gates"]), A.put(ci["c_prev"]) if with_cp else None
        c, h, act = A.new((B, H), F32), A.new((B, H), F32), A.new((B, 4 * H), F32)
        C.lstm_cell_fwd(gates, cp, c, h, act)
        assert A.ok(), case
        o = rc.cell_fwd(ci, with_cp)
        _bound("cell_fwd", case + "-acts", act, o["acts"])
        _bound("cell_fwd", case + "-c", c, o["c"])
        _bound("cell_fwd", case + "-h", h, o["h"])
        acts, ct = A.put(ci["acts"]), A.put(ci["c_t"])
        dh, dcn = A.put(ci["dh"]) if with_dh else None, A.put(ci["dc"]) if with_dc else None
        dg, dcp = A.new((B, 4 * H), F32), A.new((B, H), F32)
        C.lstm_cell_bwd(acts, cp, ct, dh, dcn, dg, dcp)
        assert A.ok(), case
        o = rc.cell_bwd(ci, with_cp, with_dh, with_dc)
        _bound("cell_bwd", case + "-dg", dg, o["dg"])
        _bound("cell_bwd", case + "-dc", dcp, o["dc"])


# ================================================================================================== 5. dropout
@pytest.mark.parametrize("off_kind", ["zero", "one_block", "step", "high_word"])
@pytest.mark.parametrize("B,T,I,H,p", rc.DROP_SHAPES)
def test_lstm_drop_rep_bit_for_bit_and_its_backward(B, T, I, H, p, off_kind):
    C = _n()
    seed = 0x1234567887654321 & 0x7FFFFFFFFFFFFFFF
    mul = 1.0 / (1.0 - p)
    g = rc.gen(70 + B + I)
    # the input sequence (K = I over T steps) and one step's hidden state (K = H, T = 1), fp32 and bf16 sources
    for K, TT, xdt, ones in ((I, T, F32, True), (I, T, BF, False), (H, 1, F32, False)):
        # a counter offset: none; one Philox block (4 ids: every draw moves to the next counter); a later step's (a
        # multiple of one step's 4 B K ids); one whose ids cross 2^34, where the Philox counter's high word starts to
        # count. The kernels take whole blocks only: bigdl_lstm_drop_rep / _bwd refuse (off & 3) != 0 before any
        # launch (one draw serves 4 consecutive ids of a row), see test_lstm_drop_rep_refuses_an_offset_inside_a_block
        off = {"zero": 0, "one_block": 4, "step": 3 * 4 * B * K,
               "high_word": (1 << 34) - 4 * ((2 * TT * B * K) // 4)}[off_kind]
        assert off % 4 == 0
        Kp = K + 4 if ones else K
        case = f"B{B}-T{TT}-K{K}-p{p}-{off_kind}-{'bf16' if xdt == BF else 'f32'}"
        x = torch.randn(B, TT, K, generator=g).to(xdt)
        keep = rc.drop_keep(seed, off, B, TT, K, p)
        assert 0 < int(keep.sum()) < keep.numel()
        A = _Arena()
        xd, y = A.put(x), A.new((4, TT * B, Kp), BF)
        C.lstm_drop_rep(xd, TT * K, K, y, TT * B * Kp, B, TT, K, Kp, ones, p, mul, seed, off)
        assert A.ok(), case
        assert rc.same_bits(y.cpu(), rc.drop_rep_oracle(x, keep, mul, Kp, ones)), case
        dy = torch.randn(4, TT * B, K, generator=g)
        for add in (None, torch.randn(B, TT, K, generator=g)):
            dyd, dx, addd = A.put(dy), A.new((B, TT, K), F32), A.put(add)
            C.lstm_drop_rep_bwd(dyd, TT * B * K, K, dx, TT * K, K, addd, TT * K, K, B, TT, K, p, mul, seed, off)
            assert A.ok(), case
            _bound("drop_bwd", case + ("-add" if add is not None else ""), dx, rc.drop_rep_bwd_oracle(dy, keep, mul, add))


def test_lstm_drop_rep_refuses_an_offset_inside_a_block():
    """A counter offset that is no multiple of 4 would split a row's draws across Philox blocks: both bindings raise
    and launch nothing (the outputs keep their sentinel bytes)."""
    C = _n()
    B, T, K = 3, 2, 8
    A = _Arena()
    x, y = A.put(torch.randn(B, T, K, generator=rc.gen(9))), A.new((4, T * B, K), BF)
    dy, dx = A.put(torch.randn(4, T * B, K, generator=rc.gen(10))), A.new((B, T, K), F32)
    for off in (1, 2, 3, 6):
        with pytest.raises(RuntimeError):
            C.lstm_drop_rep(x, T * K, K, y, T * B * K, B, T, K, K, False, 0.5, 2.0, 7, off)
        with pytest.raises(RuntimeError):
            C.lstm_drop_rep_bwd(dy, T * B * K, K, dx, T * K, K, None, T * K, K, B, T, K, 0.5, 2.0, 7, off)
    assert A.ok() and _untouched(y) and _untouched(dx)


# ================================================================================================== 6. weight gradient
@pytest.mark.parametrize("T,B,H", rc.WGRAD_SHAPES)
def test_recurrent_weight_gradient(T, B, H):
    """dU of the real _LSTMSeq backward against the fp64 product of the kernel's own dg16 and h16[:T]: the operands are
    taken where the backward hands them to its weight-gradient kernel. (3, 9, 256) runs the persistent kernels and
    their whole-sequence route, (2, 37, 96) the step kernels and _rnn_param_grads. At these row counts both routes
    end in conv2d_wgrad (the native-GEMM and hipBLASLt shape rules need more rows): that is the only weight-gradient
    kernel this test covers, and a change of the routing at these shapes fails it by name."""
    from bigdl_amd import ops
    from bigdl_amd.nn import recurrent as rec
    from bigdl_amd.ops import conv as cv

    C = _n()
    seq = bool(C.lstm_seq_supported(B, H))
    g = rc.gen(80 + B)
    xg = torch.randn(B, T, 4 * H, generator=g)
    h0, c0 = torch.randn(B, H, generator=g) * 0.5, torch.randn(B, H, generator=g) * 0.5
    U = (torch.randn(4 * H, H, generator=g) / H ** 0.5).to(BF).float()
    go = torch.randn(B, T, H, generator=g)
    seen = []
    orig_wgrad, orig_gemm = cv.conv2d_wgrad, ops.gemm.gemm

    def spy_wgrad(dy, x, dw, *a, **k):
        seen.append(("conv2d_wgrad", dy.detach().clone(), x.detach().clone()))
        return orig_wgrad(dy, x, dw, *a, **k)

    def spy_gemm(*a, **k):
        seen.append(("native_gemm", None, None))
        return orig_gemm(*a, **k)

    cv.conv2d_wgrad, ops.gemm.gemm = spy_wgrad, spy_gemm
    try:
        dev = [t.to(DEV).requires_grad_(True) for t in (xg, h0, c0, U)]
        out, hT, cT = rec._LSTMSeq.apply(*dev)
        torch.autograd.backward([out], [go.to(DEV)])
        torch.cuda.synchronize()
    finally:
        cv.conv2d_wgrad, ops.gemm.gemm = orig_wgrad, orig_gemm
    route = ("whole-sequence" if seq else "step") + ":" + "+".join(n for n, _, _ in seen)
    assert [n for n, _, _ in seen] == ["conv2d_wgrad"], f"the weight gradient took another route: {route}"
    _, dy, x = seen[0]
    dg16, h16 = dy.view(T, B, 4 * H).cpu(), x.view(T, B, H).cpu()
    assert dg16.dtype == BF and h16.dtype == BF and rc.same_bits(h16[0], h0.to(BF))
    assert float(dg16.float().abs().max()) > 0
    _bound("wgrad", f"T{T}-B{B}-H{H}-{route}", dev[3].grad, rc.wgrad_oracle(dg16, h16))
